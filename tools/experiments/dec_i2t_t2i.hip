// PARKED EXPERIMENT (round 5): image -> tokens of a decoder layer FUSED with the tokens -> image attention that follows it.
//
// Built, parity-tested against the two launches it replaces (test_dec_i2t_t2i.py next to this file) and measured SLOWER: 2.0 ms per
// 1 024-prompt layer pair against 0.81 + 0.47 ms, because its registers allow one wave per SIMD only.  Not compiled:
// saber_amd/csrc/Makefile builds nothing in this directory.  This file is a SECTION of saber_amd/csrc/decoder_fused.hip, not a translation
// unit: it uses that file's helpers (kswz, tr_read_d, cat4_d, pack8_d, I2TCfg, I2T_* / T2I_* constants) and is pasted back between
// launch_dec_i2t and the "upscaling head" section.  README.md in this directory lists the steps; the pieces that lived in other files are
// kept at the end of this one.

// ------------------------------------------------------------------------------------------------ image -> tokens of layer l FUSED with the
// tokens -> image attention that follows it (round 5; VERDICT r01-r04 "i2t + next-t2i")
// X' = LN(X + softmax((X + pe).Kt).Vt + b_o) is written to HBM as before, and every pair of finished 16-row tiles is at once the next
// attention's key / value block: the 2 MB of X' per prompt are NOT read back by a separate dec_t2i launch.  The queries of that
// attention depend on the tokens only (dec_tokens_kernel has produced fold_q / tq before this kernel runs).
// Structure: dec_i2t_kernel<1>'s tile loop unchanged (4 waves = the four 16-column quarters of the score matrix, one barrier per tile),
// plus, per wave, ONE 16-row query tile of the next attention (wave = q tile): finish_tile also drops the normalised rows into `xbuf`
// (dec_t2i's tile format: 512-B rows, 16-byte chunks XOR-swizzled by row & 15), four tiles deep, and every second iteration the wave
// runs dec_t2i's block step on the 32 keys of the pair finished two iterations earlier (18 + 16 MFMAs, online softmax).  The PEK rows of
// a pair come global -> LDS directly, two wave-instructions per wave and pair, two stages.
// Registers: dec_i2t's ~200 + 32 (Q fragments) + 64 (partial sums) + ~16: ONE workgroup of four waves per CU (one wave per SIMD) - the
// price of the fusion, see DESIGN.md section 8.2.
#define FZ_XBUF (4 * 16 * ROW_B)                 // 32 KB: four X' tiles
#define FZ_PEK_STAGE (32 * T2I_PEK_ROWB)         // 8 KB: the PEK rows of one pair of tiles
struct I2TFuse {
    const bf16_t* pek; const bf16_t* Qt; const float* tq; float qscale; const bf16_t* Wv; const float* bv; bf16_t* out;
};
template <bool STAMPS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void dec_i2t_t2i_kernel(const bf16_t* __restrict__ X, int64_t x_bs, int x_div, int x_off, const bf16_t* __restrict__ peq,
                        const bf16_t* __restrict__ Kt, const float* __restrict__ tk, float kscale, const float* __restrict__ cb,
                        const bf16_t* __restrict__ VtT, const float* __restrict__ bo,
                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                        bf16_t* __restrict__ Xout, I2TFuse f, unsigned long long* __restrict__ stamps) {
    using CF = I2TCfg<1>;
    constexpr int I2T_ROWS = CF::ROWS, I2T_STAGE = CF::STAGE, I2T_PBUF_B = CF::PBUF_B, I2T_STAT_B = CF::STAT_B;
    constexpr int NT = 4096 / I2T_ROWS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long ts[4] = {0, 0, 0, 0}, tprev = 0;
#define FZ_STAMP(k) do { if (STAMPS) { const unsigned long long _n = __builtin_amdgcn_s_memtime(); ts[k] += _n - tprev; tprev = _n; } } while (0)
    char* pbuf = smem + I2T_NSTAGE * I2T_STAGE;
    float* stat = reinterpret_cast<float*>(pbuf + 2 * I2T_PBUF_B);
    char* xbuf = smem + CF::LDS;
    char* pkbuf = xbuf + FZ_XBUF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave;                  // i2t: score quarter;  t2i: query tile
    const int fi = lane & 15, fg = lane >> 4;
    const int p = blockIdx.x;
    const bf16_t* Xp = X + (int64_t)((p + x_off) / x_div) * x_bs;
    bf16_t* Xo = Xout + (int64_t)p * 4096 * DC;

    // ---- i2t operands (dec_i2t_kernel)
    op16x8 kf[8], vf[4][2];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
        kf[ks] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(Kt + ((int64_t)p * 64 + 16 * qr + fi) * DC + 32 * ks + 8 * fg));
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            vf[t][ks] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(VtT + ((int64_t)p * 256 + 64 * qr + 16 * t + fi) * 64 + 32 * ks + 8 * fg));
    op16x8 kq;
    {
        const int hsel = fg >> 1;
        const float* kp = tk + ((int64_t)p * 8 + (fi & 7)) * 128 + 16 * (2 * qr + hsel) + 8 * (fg & 1);
        const float4 a = *reinterpret_cast<const float4*>(kp), b = *reinterpret_cast<const float4*>(kp + 4);
        const float z = ((fi >> 3) == hsel) ? kscale : 0.f;
        kq = pack8_d(a.x * z, a.y * z, a.z * z, a.w * z, b.x * z, b.y * z, b.z * z, b.w * z);
    }
    const float4 cb4 = *reinterpret_cast<const float4*>(cb + (int64_t)p * 64 + 16 * qr + 4 * fg);
    f32x2 g2[8], be2[8], bo2[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float4 b4 = *reinterpret_cast<const float4*>(bo + 64 * qr + 16 * t + 4 * fg);
        const float4 g4 = *reinterpret_cast<const float4*>(gamma + 64 * qr + 16 * t + 4 * fg);
        const float4 e4 = *reinterpret_cast<const float4*>(beta + 64 * qr + 16 * t + 4 * fg);
        g2[2 * t] = (f32x2){g4.x, g4.y}; g2[2 * t + 1] = (f32x2){g4.z, g4.w};
        be2[2 * t] = (f32x2){e4.x, e4.y}; be2[2 * t + 1] = (f32x2){e4.z, e4.w};
        bo2[2 * t] = (f32x2){b4.x, b4.y}; bo2[2 * t + 1] = (f32x2){b4.z, b4.w};
    }
    // ---- t2i operands of this wave's query tile (dec_t2i_kernel, qt = wave)
    op16x8 qf[8], pq;
    {
        const bf16_t* qrow = f.Qt + ((int64_t)p * 64 + qr * 16 + fi) * DC;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[ks] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(qrow + 32 * ks + 8 * fg));
        const int hsel = fg >> 1;
        const float* qp = f.tq + ((int64_t)p * 8 + (fi & 7)) * 128 + 16 * (2 * qr + hsel) + 8 * (fg & 1);
        const float4 a = *reinterpret_cast<const float4*>(qp), b = *reinterpret_cast<const float4*>(qp + 4);
        const float z = ((fi >> 3) == hsel) ? f.qscale : 0.f;
        pq = pack8_d(a.x * z, a.y * z, a.z * z, a.w * z, b.x * z, b.y * z, b.z * z, b.w * z);
    }
    float m = -3.0e38f, l = 0.f;
    f32x4 o[16];
#pragma unroll
    for (int dt = 0; dt < 16; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- LDS-DMA: per tile 2 X pieces + 1 PEQ piece per wave (dec_i2t_kernel), per PAIR of tiles 2 PEK pieces per wave
    int srow[2], schunk[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        srow[i] = 2 * (wave * 2 + i) + (lane >> 5);
        schunk[i] = (lane & 31) ^ (srow[i] & 15);
    }
    const int prow = 4 * wave + (lane >> 4), pchunk = (lane & 15) ^ (prow & 15);
    auto issue = [&](int t) {
        char* sx = smem + (t & (I2T_NSTAGE - 1)) * I2T_STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t off = (int64_t)(t * I2T_ROWS + srow[i]) * DC + schunk[i] * 8;
            if (x_div > 1) __builtin_amdgcn_global_load_lds((gptr_d)(Xp + off), (lptr_d)(sx + (wave * 2 + i) * 1024), 16, 0, 0);
            else __builtin_amdgcn_global_load_lds((gptr_d)(Xp + off), (lptr_d)(sx + (wave * 2 + i) * 1024), 16, 0, I2T_X_AUX);
        }
        __builtin_amdgcn_global_load_lds((gptr_d)(peq + (int64_t)(t * I2T_ROWS + prow) * 128 + pchunk * 8), (lptr_d)(sx + I2T_ROWS * ROW_B + wave * 1024), 16, 0, 0);
    };
    int krow[2], kchunk[2];          // PEK: 32 rows x 256 B = 8 pieces of 4 rows; wave w issues pieces 2w, 2w + 1
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        krow[i] = 4 * (wave * 2 + i) + (lane >> 4);
        kchunk[i] = (lane & 15) ^ (krow[i] & 15);
    }
    auto issue_pek = [&](int pair) {             // the PEK rows of tiles 2 pair, 2 pair + 1
        char* sk = pkbuf + (pair & 1) * FZ_PEK_STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((gptr_d)(f.pek + (int64_t)(pair * 32 + krow[i]) * 128 + kchunk[i] * 8), (lptr_d)(sk + (wave * 2 + i) * 1024), 16, 0, 0);
    };
    const int poff = fi * I2T_PEQ_ROWB + (((4 * qr + fg) ^ fi) << 4);
    int xoff[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) xoff[ks] = fi * ROW_B + (((4 * ks + fg) ^ fi) << 4);
    int roff[4];      // this lane's 8-byte pieces of row fi: channels 64 qr + 16 t + 4 fg .. + 3, in the swizzled tile format
#pragma unroll
    for (int t = 0; t < 4; ++t) roff[t] = fi * ROW_B + (((8 * qr + 2 * t + (fg >> 1)) ^ fi) << 4) + (fg & 1) * 8;
    const uint32_t prow_a = (uint32_t)(uintptr_t)(lptr_d)(pbuf + fi * I2T_PSTRIDE);
    const uint32_t stat_a = (uint32_t)(uintptr_t)(lptr_d)(stat + (fi * 4) * 2);
    const uint32_t smem_a = (uint32_t)(uintptr_t)(lptr_d)smem;
    const uint32_t oscr_a = smem_a + I2T_NSTAGE * I2T_STAGE + 2 * I2T_PBUF_B + 2 * I2T_STAT_B + wave * 2048;
    const uint32_t xbuf_a = (uint32_t)(uintptr_t)(lptr_d)xbuf;
    f32x2 y2[8];
    auto finish_tile = [&](int tp) {
        f32x4 a, b;
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(stat_a + (tp & 1) * I2T_STAT_B) : "memory");
        const float tot = (a.x + a.z) + (b.x + b.z), tsq = (a.y + a.w) + (b.y + b.w);
        const float mean = tot * (1.0f / DC);
        const float rstd = __builtin_amdgcn_rsqf(fmaxf(tsq * (1.0f / DC) - mean * mean, 0.f) + eps);
        const f32x2 mean2 = (f32x2){mean, mean}, rstd2 = (f32x2){rstd, rstd};
        const uint32_t tb = oscr_a + fi * 128 + (fg & 1) * 8;
        const uint32_t xb = xbuf_a + (tp & 3) * (16 * ROW_B);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const f32x2 v0 = ((y2[2 * tt] - mean2) * rstd2) * g2[2 * tt] + be2[2 * tt];
            const f32x2 v1 = ((y2[2 * tt + 1] - mean2) * rstd2) * g2[2 * tt + 1] + be2[2 * tt + 1];
            const uint32_t lo = pack_op16(v0.x, v0.y), hi = pack_op16(v1.x, v1.y);
            lds_write_b64(tb + (((2 * tt + (fg >> 1)) ^ (fi & 7)) << 4), lo, hi);
            lds_write_b64(xb + roff[tt], lo, hi);            // the next attention's key / value tile
        }
        u32x4 o0, o1;
        asm volatile("s_waitcnt lgkmcnt(0)\n\tds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(o0), "=&v"(o1) : "v"(oscr_a + (lane >> 3) * 128 + (((lane & 7) ^ ((lane >> 3) & 7)) << 4)) : "memory");
        bf16_t* orow = Xo + (int64_t)(tp * I2T_ROWS + (lane >> 3)) * DC + 64 * qr + 8 * (lane & 7);
        __builtin_nontemporal_store(o0, reinterpret_cast<u32x4*>(orow));
        __builtin_nontemporal_store(o1, reinterpret_cast<u32x4*>(orow + 8 * DC));
    };
    // dec_t2i_kernel's block step on the 32 keys of tiles 2 pair, 2 pair + 1 (this wave's 16 query rows)
    int koff[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) koff[ks] = fi * ROW_B + (((4 * ks + fg) ^ fi) << 4);
    const int vrow = 4 * fg + (fi >> 2);
    const int vsel = (fi & 3) >> 1, vlow = (fi & 1) * 8;
    auto t2i_step = [&](int pair) {
        const uint32_t xs = xbuf_a + (pair & 1) * (32 * ROW_B);
        const uint32_t ps = (uint32_t)(uintptr_t)(lptr_d)pkbuf + (pair & 1) * FZ_PEK_STAGE;
        f32x4 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            op16x8 kp, kx[8];
            asm volatile("ds_read_b128 %0, %1" : "=v"(kp) : "v"(ps + (kt * 16 + fi) * T2I_PEK_ROWB + (((4 * qr + fg) ^ fi) << 4)) : "memory");
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) asm volatile("ds_read_b128 %0, %1" : "=v"(kx[ks]) : "v"(xs + kt * 16 * ROW_B + koff[ks]) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kp), "+v"(kx[0]), "+v"(kx[1]), "+v"(kx[2]), "+v"(kx[3]), "+v"(kx[4]), "+v"(kx[5]), "+v"(kx[6]), "+v"(kx[7]));
            s[kt] = MFMA_16x16x32(kp, pq, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) s[kt] = MFMA_16x16x32(kx[ks], qf[ks], s[kt], 0, 0, 0);
        }
        float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
        mx = xor32_max(xor16_max(mx));
        if (__any(mx > m)) {
            const float mn = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            l *= alpha;
#pragma unroll
            for (int dt = 0; dt < 16; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        }
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[kt][r] - m);
                s[kt][r] = e;
                sum += e;
            }
        sum = xor32_sum(xor16_sum(sum));
        l += sum;
        const op16x8 pf = pack8_d(s[0][0], s[0][1], s[0][2], s[0][3], s[1][0], s[1][1], s[1][2], s[1][3]);
        const uint32_t va = xs + vrow * ROW_B + vlow;
#pragma unroll
        for (int d4 = 0; d4 < 16; d4 += 4) {
            u32x2_d lo[4], hi[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int sw = ((2 * (d4 + j) + vsel) ^ (vrow & 15)) << 4;
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo[j]) : "v"(va + sw) : "memory");
                asm volatile("ds_read_b64_tr_b16 %0, %1 offset:8192" : "=v"(hi[j]) : "v"(va + sw) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const op16x8 vfr = cat4_d(__builtin_bit_cast(op16x4, lo[j]), __builtin_bit_cast(op16x4, hi[j]));
                o[d4 + j] = MFMA_16x16x32(vfr, pf, o[d4 + j], 0, 0, 0);
            }
        }
    };

    issue(0); issue(1); issue(2);
    issue_pek(0);
    // queue of this wave: L(0) L(1) L(2) K(0); tile 0 must have landed
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (STAMPS) tprev = __builtin_amdgcn_s_memtime();
    for (int t = 0; t < NT; ++t) {
        const char* xs = smem + (t & (I2T_NSTAGE - 1)) * I2T_STAGE;
        const char* ps = xs + I2T_ROWS * ROW_B;
        f32x4 s = (f32x4){cb4.x, cb4.y, cb4.z, cb4.w}, s1;
        {
            const op16x8 pf = *reinterpret_cast<const op16x8*>(ps + poff);
            s1 = MFMA_16x16x32(kq, pf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 8; ks += 2) {
            const op16x8 xf0 = *reinterpret_cast<const op16x8*>(xs + xoff[ks]);
            const op16x8 xf1 = *reinterpret_cast<const op16x8*>(xs + xoff[ks + 1]);
            s = MFMA_16x16x32(kf[ks], xf0, s, 0, 0, 0);
            s1 = MFMA_16x16x32(kf[ks + 1], xf1, s1, 0, 0, 0);
        }
        s += s1;
        {
            float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
            mx = xor16_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[r] = __builtin_amdgcn_exp2f(s[r] - mx); sum += s[r]; }
            sum = xor16_sum(sum);
            const float inv = __builtin_amdgcn_rcpf(sum);
            lds_write_b64(prow_a + (t & 1) * I2T_PBUF_B + (16 * qr + 4 * fg) * 2, pack_op16(s[0] * inv, s[1] * inv), pack_op16(s[2] * inv, s[3] * inv));
        }
        FZ_STAMP(0);
        // Tile t + 1 must have landed before the barrier publishes it.  After its barrier iteration i issues L(i + 3) [3 operations],
        // S(i - 1) [2 stores] and, when i is even and >= 2, K(i / 2) [2] - the PEK rows of the pair that is consumed in iteration i + 3, into
        // the stage that the step of iteration i - 1 has read (every wave is past that step: this iteration's barrier).  Behind L(t + 1) in
        // this wave's queue: S(t - 3), L(t + 2), S(t - 2) and exactly one K: 9 operations may stay in flight.  The PEK rows an odd
        // iteration consumes were issued BEFORE L(t + 1) (iteration t - 3), so the same wait covers them.
        if (t + 3 >= NT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (t < 3) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");            // t = 0: L(2) K(0);  t = 1: K(0) L(3);  t = 2: L(4) S(0)
        else asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        FZ_STAMP(1);
        if (t + 3 < NT) issue(t + 3);
        if (t > 0) finish_tile(t - 1);
        // the pair (t - 3, t - 2): both tiles were dropped into xbuf before this iteration's barrier
        if ((t & 1) && t >= 3) t2i_step((t - 3) >> 1);
        else if (!(t & 1) && t >= 2) issue_pek(t >> 1);
        FZ_STAMP(2);
        f32x4 y[4];
        {
            op16x8 p0, p1;
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:64\n\ts_waitcnt lgkmcnt(0)" : "=&v"(p0), "=&v"(p1) : "v"(prow_a + (t & 1) * I2T_PBUF_B + 16 * fg) : "memory");
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                y[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                y[tt] = MFMA_16x16x32(vf[tt][0], p0, y[tt], 0, 0, 0);
                y[tt] = MFMA_16x16x32(vf[tt][1], p1, y[tt], 0, 0, 0);
            }
        }
        uint64_t xr0, xr1, xr2, xr3;
        {
            const uint32_t xa = smem_a + (t & (I2T_NSTAGE - 1)) * I2T_STAGE;
            asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %5\n\tds_read_b64 %2, %6\n\tds_read_b64 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(xr0), "=&v"(xr1), "=&v"(xr2), "=&v"(xr3)
                         : "v"(xa + roff[0]), "v"(xa + roff[1]), "v"(xa + roff[2]), "v"(xa + roff[3])
                         : "memory");
        }
        const uint64_t xrs[4] = {xr0, xr1, xr2, xr3};
        f32x2 sum2 = (f32x2){0.f, 0.f}, sq2 = (f32x2){0.f, 0.f};
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const uint32_t xlo = (uint32_t)xrs[tt], xhi = (uint32_t)(xrs[tt] >> 32);
            const f32x2 r0 = (f32x2){op16_lo(xlo), op16_hi(xlo)};
            const f32x2 r1 = (f32x2){op16_lo(xhi), op16_hi(xhi)};
            y2[2 * tt] = ((f32x2){y[tt][0], y[tt][1]} + bo2[2 * tt]) + r0;
            y2[2 * tt + 1] = ((f32x2){y[tt][2], y[tt][3]} + bo2[2 * tt + 1]) + r1;
            sum2 += y2[2 * tt]; sum2 += y2[2 * tt + 1];
            sq2 = __builtin_elementwise_fma(y2[2 * tt], y2[2 * tt], sq2);
            sq2 = __builtin_elementwise_fma(y2[2 * tt + 1], y2[2 * tt + 1], sq2);
        }
        float sum = sum2.x + sum2.y, sq = sq2.x + sq2.y;
        sum = xor16_sum(sum); sq = xor16_sum(sq);
        sum = xor32_sum(sum); sq = xor32_sum(sq);
        if (fg == 0) lds_write_b64(stat_a + (t & 1) * I2T_STAT_B + qr * 8, __float_as_uint(sum), __float_as_uint(sq));
        FZ_STAMP(3);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    finish_tile(NT - 1);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the loop's last step (t = NT - 1) took the pair (NT - 4, NT - 3); the last pair is left
    t2i_step(NT / 2 - 1);
    if (STAMPS && stamps && lane == 0)
        for (int k = 0; k < 4; ++k) stamps[((int64_t)blockIdx.x * 4 + wave) * 4 + k] = ts[k];
    // ---- normalise and apply v_proj (dec_t2i_kernel's tail for a whole key range in one workgroup): out[p][t][16 h + i]
    __syncthreads();
    float* mo = reinterpret_cast<float*>(smem) + (size_t)qr * 16 * 260;
    {
        const float inv = __builtin_amdgcn_rcpf(l);
#pragma unroll
        for (int dt = 0; dt < 16; ++dt)
            *reinterpret_cast<float4*>(mo + fi * 260 + 16 * dt + 4 * fg) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
        __builtin_amdgcn_wave_barrier();
        f32x4 r0 = (f32x4){0.f, 0.f, 0.f, 0.f}, r1 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const float4 z0 = *reinterpret_cast<const float4*>(mo + fi * 260 + 32 * ks + 8 * fg), z1 = *reinterpret_cast<const float4*>(mo + fi * 260 + 32 * ks + 8 * fg + 4);
            const op16x8 zf = pack8_d(z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w);
            const op16x8 w0 = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(f.Wv + (int64_t)(32 * qr + fi) * DC + 32 * ks + 8 * fg));
            const op16x8 w1 = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(f.Wv + (int64_t)(32 * qr + 16 + fi) * DC + 32 * ks + 8 * fg));
            r0 = MFMA_16x16x32(w0, zf, r0, 0, 0, 0);
            r1 = MFMA_16x16x32(w1, zf, r1, 0, 0, 0);
        }
        const int hsel = fi >> 3, hh = 2 * qr + hsel, tt = fi & 7;
        const float4 b4 = *reinterpret_cast<const float4*>(f.bv + 16 * hh + 4 * fg);
        const f32x4 r = hsel ? r1 : r0;
        *reinterpret_cast<uint2*>(f.out + (int64_t)p * 1024 + tt * 128 + 16 * hh + 4 * fg) =
            make_uint2(pack_op16(r[0] + b4.x, r[1] + b4.y), pack_op16(r[2] + b4.z, r[3] + b4.w));
    }
#undef FZ_STAMP
}

const char* launch_dec_i2t_t2i(const bf16_t* X, XMap xm, const bf16_t* peq, const bf16_t* Kt, const float* tk, float kscale, const float* cb, const bf16_t* VtT,
                               const float* bo, const float* gamma, const float* beta, float eps, bf16_t* Xout, int P,
                               const bf16_t* pek, const bf16_t* Qt, const float* tq, float qscale, const bf16_t* Wv, const float* bv, bf16_t* out, hipStream_t s) {
    if (P <= 0) return nullptr;
    if (xm.div <= 0) return "dec_i2t_t2i: XMap.div must be positive";
    const I2TFuse f{pek, Qt, tq, qscale, Wv, bv, out};
    constexpr int lds = I2TCfg<1>::LDS + FZ_XBUF + 2 * FZ_PEK_STAGE;
    static_assert(lds >= 4 * 16 * 260 * 4, "the v_proj tail re-uses the front of the LDS");
    if (g_saber_stamp_buf)
        hipLaunchKernelGGL((dec_i2t_t2i_kernel<true>), dim3(P), dim3(256), lds, s, X, xm.stride, xm.div, xm.off, peq, Kt, tk, kscale, cb, VtT, bo, gamma, beta, eps, Xout, f, g_saber_stamp_buf);
    else
        hipLaunchKernelGGL((dec_i2t_t2i_kernel<false>), dim3(P), dim3(256), lds, s, X, xm.stride, xm.div, xm.off, peq, Kt, tk, kscale, cb, VtT, bo, gamma, beta, eps, Xout, f, (unsigned long long*)nullptr);
    return nullptr;
}

// ---- the rest of the experiment, as it stood in the other files ----
//
// decoder_fused.hip, decoder_fused_init_device(), after the dec_t2i_w1_kernel lines:
//
//    if (st == hipSuccess) st = hipFuncSetAttribute(reinterpret_cast<const void*>(dec_i2t_t2i_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, I2TCfg<1>::LDS + FZ_XBUF + 2 * FZ_PEK_STAGE);
//    if (st == hipSuccess) st = hipFuncSetAttribute(reinterpret_cast<const void*>(dec_i2t_t2i_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, I2TCfg<1>::LDS + FZ_XBUF + 2 * FZ_PEK_STAGE);
//
// kernels_op.h, after launch_dec_i2t (and SABER_OP_FWD(launch_dec_i2t_t2i) in kernels.h):
//
//    // dec_i2t of layer l fused with the tokens -> image attention that follows it (round 5): X' is written as before and consumed as the next
//    // attention's keys / values from LDS; `out` = that attention's output after v_proj (what launch_dec_t2i writes).  P workgroups of four waves.
//    const char* launch_dec_i2t_t2i(const bf16_t* X, XMap xm, const bf16_t* peq, const bf16_t* Kt, const float* tk, float kscale, const float* cb, const bf16_t* VtT,
//                                   const float* bo, const float* gamma, const float* beta, float eps, bf16_t* Xout, int P,
//                                   const bf16_t* pek, const bf16_t* Qt, const float* tq, float qscale, const bf16_t* Wv, const float* bv, bf16_t* out, hipStream_t s);
//
// engine.hip, decode_chunk, after the run_i2t lambda (8-row route; the two `TRY(run_i2t(..)); TRY(run_t2i(..));` pairs behind segments S1 and
// S2 become TRY(run_i2t_t2i(e->dl[0], e->dl[1].t2i)) and TRY(run_i2t_t2i(e->dl[1], e->final_attn))):
//
//    // Opt-in (round 5, SABER_AMD_FUSE_I2T_T2I=1, read per call): image -> tokens of a layer and the tokens -> image attention that follows
//    // it in ONE kernel (dec_i2t_t2i_kernel: X' is the next attention's key / value block while it is still in LDS).  Same results as the
//    // two launches up to the order of the online softmax; measured slower (one wave per SIMD): DESIGN.md section 8.2.
//    const bool fuse = getenv("SABER_AMD_FUSE_I2T_T2I") != nullptr && P >= 128;
//    auto run_i2t_t2i = [&](const DecLayerW& w, const AttnW& a) -> int {
//        if (!fuse || build != nullptr) { TRY(run_i2t(w)); return run_t2i(a); }
//        ENG_KP(e, PC_DEC_I2T, 8.0 * 64 * 4096.0 * 256 * P, (double)P * 4096 * 256 * 4,
//               launch_dec_i2t_t2i(X, xm, w.i2t.pe_proj, e->fold_k, e->tk, kScale, e->fold_cb, e->fold_v, w.i2t.o.b, w.n4.g, w.n4.b, 1e-5f, e->keys_bf, P,
//                                  a.pe_proj, e->fold_q, e->tq, kScale, a.v.w, a.v.b, e->t_att, s));
//        X = e->keys_bf; xm = per_prompt; build = nullptr;
//        return SABER_OK;
//    };
