// Kernel-level C-ABI (include/saber_amd_kernels.h): thin wrappers over the launchers.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/saber_amd_kernels.h"
#include "common.h"
#include "kernels.h"
#include "engine.h"
#include "exact.h"

#include <atomic>

static thread_local std::string g_kerr;
static int kfail(const char* m) { g_kerr = m ? m : "unknown"; return -1; }
static int kcheck(const char* m) {
    if (m) return kfail(m);
    hipError_t st = hipGetLastError();
    if (st != hipSuccess) return kfail(hipGetErrorString(st));
    return 0;
}

extern "C" const char* saber_k_last_error(void) { return g_kerr.c_str(); }

extern "C" int saber_k_init(int device_id) {
    if (hipSetDevice(device_id) != hipSuccess) return kfail("hipSetDevice failed");
    const char* m = gemm_init_device();
    if (!m) m = gemm_rowln_init_device();
    if (!m) m = gemm_mlp_rowln_init_device();
    if (!m) m = hiera_attention_init_device();
    if (!m) m = image_ops_init_device();
    if (!m) m = decoder_fused_init_device();
    if (!m) m = decoder_t16_init_device();
    if (!m) m = amg_device_init();
    (void)hipGetLastError();
    if (m) return kfail(m);
    return 0;
}

extern "C" int saber_k_gemm(const uint16_t* A, const uint16_t* W, const float* bias, const float* res, float* out_f32,
                            uint16_t* out_bf16, int M, int N, int K, int act, int act_last, int pool4, int res_shift, int res_mod,
                            void* stream) {
    GemmParams p;
    p.A = A; p.lda = K; p.W = W; p.ldw = K; p.bias = bias; p.res = res; p.ldres = N; p.Cf = out_f32; p.ldcf = N; p.Cb = out_bf16; p.ldcb = N;
    p.M = M; p.N = N; p.K = K; p.act = act; p.act_last = act_last; p.pool4 = pool4; p.res_shift = res_shift; p.res_mod = res_mod;
    return kcheck(launch_gemm(p, (hipStream_t)stream));
}

extern "C" int saber_k_gemm_ld(const uint16_t* A, int lda, const uint16_t* W, int ldw, int w_kpad, const float* bias, const float* res,
                               float* out_f32, uint16_t* out_bf16, int M, int N, int K, int act, void* stream) {
    GemmParams p;
    p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.bias = bias; p.res = res; p.ldres = N; p.Cf = out_f32; p.ldcf = N; p.Cb = out_bf16; p.ldcb = N;
    p.M = M; p.N = N; p.K = K; p.act = act; p.w_kpad = w_kpad;
    // the widest 16-bit-output GEMMs read W packed per K-step (the engine packs qkv / mlp.layers.0 once at finalize: engine.hip); here: into a
    // scratch kept per thread, so that the kernel-level tests and tools/gemm_bench.py reach the kernels the engine runs
    if (w_kpad && out_bf16 && !out_f32 && !res && (K % 64) == 0 && (N & 7) == 0 && ((int64_t)M * N >= (int64_t)1024 * 65536 || (g_saber_debug_flags & 128))) {
        static thread_local bf16_t* scratch = nullptr;
        static thread_local size_t scratch_elems = 0;
        const size_t need = gemm_rowln_packed_elems(N, K);
        if (need > scratch_elems) {
            if (scratch) { (void)hipDeviceSynchronize(); (void)hipFree(scratch); scratch = nullptr; scratch_elems = 0; }
            if (hipMalloc(reinterpret_cast<void**>(&scratch), need * sizeof(bf16_t)) != hipSuccess) return kfail("gemm: scratch allocation failed");
            scratch_elems = need;
        }
        if (const char* m = launch_pack_w_kstep(W, ldw, N, K, scratch, (hipStream_t)stream)) return kfail(m);
        p.Wpk = scratch;
    }
    return kcheck(launch_gemm(p, (hipStream_t)stream));
}

extern "C" int saber_k_gemm_rowln(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* res, float* out_f32,
                                  uint16_t* out_bf16, const float* ln_gamma, const float* ln_beta, float ln_eps, uint16_t* ln_out, int M, int N, int K,
                                  void* stream) {
    // the kernel reads W packed per K-step (the engine packs its weights once at finalize); here: into a scratch kept per thread
    static thread_local bf16_t* scratch = nullptr;
    static thread_local size_t scratch_elems = 0;
    const size_t need = gemm_rowln_packed_elems(N, K);
    if (need > scratch_elems) {
        if (scratch) { (void)hipDeviceSynchronize(); (void)hipFree(scratch); scratch = nullptr; scratch_elems = 0; }
        if (hipMalloc(reinterpret_cast<void**>(&scratch), need * sizeof(bf16_t)) != hipSuccess) return kfail("gemm_rowln: scratch allocation failed");
        scratch_elems = need;
    }
    if (const char* m = launch_pack_w_kstep(W, ldw, N, K, scratch, (hipStream_t)stream)) return kfail(m);
    GemmParams p;
    p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.w_kpad = 1; p.bias = bias; p.res = res; p.ldres = N; p.Cf = out_f32; p.ldcf = N; p.Cb = out_bf16; p.ldcb = N;
    p.M = M; p.N = N; p.K = K; p.ln_gamma = ln_gamma; p.ln_beta = ln_beta; p.ln_eps = ln_eps; p.ln_out = ln_out; p.ldln = N; p.Wpk = scratch;
    return kcheck(launch_gemm_rowln(p, (hipStream_t)stream));
}

extern "C" int saber_k_mlp_rowln(const uint16_t* A, int lda, const uint16_t* W1, int ldw1, const float* b1, const uint16_t* W2, int ldw2, const float* b2,
                                 const float* res, float* out_f32, uint16_t* out_bf16, const float* ln_gamma, const float* ln_beta, float ln_eps, uint16_t* ln_out,
                                 int M, int C, void* stream) {
    // the kernel reads both weights as one fragment stream (the engine packs it once at finalize); here: into a scratch kept per thread
    if (!gemm_mlp_rowln_width(C)) return kfail("mlp_rowln: width not built (C must be 144)");
    static thread_local bf16_t* scratch = nullptr;
    static thread_local size_t scratch_elems = 0;
    const size_t need = gemm_mlp_rowln_packed_elems(C);
    if (need > scratch_elems) {
        if (scratch) { (void)hipDeviceSynchronize(); (void)hipFree(scratch); scratch = nullptr; scratch_elems = 0; }
        if (hipMalloc(reinterpret_cast<void**>(&scratch), need * sizeof(bf16_t)) != hipSuccess) return kfail("mlp_rowln: scratch allocation failed");
        scratch_elems = need;
    }
    if (const char* m = launch_pack_mlp_chunks(W1, ldw1, W2, ldw2, C, scratch, (hipStream_t)stream)) return kfail(m);
    GemmParams p;
    p.A = A; p.lda = lda; p.bias1 = b1; p.bias = b2; p.res = res; p.ldres = C; p.Cf = out_f32; p.ldcf = C; p.Cb = out_bf16; p.ldcb = C;
    p.M = M; p.N = C; p.K = C; p.ln_gamma = ln_gamma; p.ln_beta = ln_beta; p.ln_eps = ln_eps; p.ln_out = ln_out; p.ldln = C; p.Wpk = scratch;
    return kcheck(launch_gemm_mlp_rowln(p, (hipStream_t)stream));
}

extern "C" int saber_k_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out_f32, uint16_t* out_bf16,
                                 int rows, int C, int act, void* stream) {
    LayerNormParams p;
    p.x = x; p.ldx = C; p.gamma = gamma; p.beta = beta; p.eps = eps; p.out_f = out_f32; p.out_bf = out_bf16; p.ldo = C; p.rows = rows; p.C = C; p.act = act;
    return kcheck(launch_layernorm(p, (hipStream_t)stream));
}

extern "C" int saber_k_hiera_attention(const uint16_t* qkv, uint16_t* out, int n_windows, int nk, int heads, int q_pool, void* stream) {
    return kcheck(launch_hiera_attention(qkv, out, n_windows, nk, heads, 72, q_pool, nullptr, (hipStream_t)stream));
}

extern "C" int saber_k_hiera_attention_ex(const uint16_t* qkv, uint16_t* out, int n_windows, int nk, int heads, int head_dim, int q_pool,
                                          const uint8_t* key_mask, void* stream) {
    return kcheck(launch_hiera_attention(qkv, out, n_windows, nk, heads, head_dim, q_pool, key_mask, (hipStream_t)stream));
}

extern "C" int saber_k_dec_attention(const float* q, const float* k, const float* v, uint16_t* out, int B, int nq, int nk, int heads,
                                     int hd, int k_shared, void* stream) {
    const int64_t C = (int64_t)heads * hd;
    return kcheck(launch_dec_attention(q, k, v, out, B, nq, nk, heads, hd, nq * C, k_shared ? 0 : nk * C, k_shared ? 0 : nk * C, nq * C,
                                       (hipStream_t)stream));
}

extern "C" int saber_k_prepare(const void* img, int dtype, int H, int W, float* out, float* ws_dev, uint32_t* minmax_dev, void* stream) {
    if (dtype == 0) return kcheck(launch_prepare_u16((const uint16_t*)img, H, W, out, ws_dev, minmax_dev, (hipStream_t)stream));
    if (dtype == 1) return kcheck(launch_prepare_f32((const float*)img, H, W, out, ws_dev, minmax_dev, (hipStream_t)stream));
    return kfail("prepare: dtype must be 0 (u16) or 1 (f32)");
}

extern "C" int saber_k_mask_post(const float* lowres, int n, int crop_x0, int crop_y0, int crop_w, int crop_h, int H, int W, float thr,
                                 float offset, uint32_t* bits, int32_t* stats, void* stream) {
    return kcheck(launch_mask_post(lowres, nullptr, n, crop_x0, crop_y0, crop_w, crop_h, H, W, thr, offset, bits,
                                   reinterpret_cast<MaskStats*>(stats), (hipStream_t)stream));
}

extern "C" int saber_k_mask_post_ex(const float* lowres, const int* idx, const uint8_t* pass, int n, int crop_x0, int crop_y0, int crop_w, int crop_h,
                                    int H, int W, float thr, float offset, uint32_t* bits, int32_t* stats, void* stream) {
    return kcheck(launch_mask_post(lowres, idx, n, crop_x0, crop_y0, crop_w, crop_h, H, W, thr, offset, bits,
                                   reinterpret_cast<MaskStats*>(stats), (hipStream_t)stream, pass));
}

extern "C" int saber_k_mask_post_group(const float* lowres, const int* idx, const uint8_t* pass, const int32_t* crops_host, const int32_t* crops_dev, int n_crops,
                                       int H, int W, float thr, float offset, uint32_t* bits, int32_t* stats, void* stream) {
    static_assert(sizeof(DevCrop) == 8 * sizeof(int32_t), "saber_k_mask_post_group: 8 int32 per crop");
    if (n_crops > 0 && (!crops_host || !crops_dev)) return kfail("mask_post_group: the crop table is needed on the host and on the device");
    return kcheck(launch_mask_post_group(lowres, idx, reinterpret_cast<const DevCrop*>(crops_dev), reinterpret_cast<const DevCrop*>(crops_host), n_crops, H, W, thr, offset,
                                         bits, reinterpret_cast<MaskStats*>(stats), (hipStream_t)stream, pass));
}

extern "C" int saber_k_resize_normalize(const float* img, int H, int W, int channels, const int* crops_dev, int n, float* out, int res, void* stream) {
    // the launcher's grid is res / 16 blocks per axis: any other res would leave a border of `out` unwritten
    if (res <= 0 || (res % 16) != 0) return kfail("resize_normalize: res must be a positive multiple of 16");
    if (n <= 0) return 0;
    return kcheck(launch_resize_normalize(img, H, W, channels, crops_dev, n, out, res, (hipStream_t)stream));
}

extern "C" int saber_k_patch_embed(const float* pix, const float* wt, const float* bias, const float* pos, float* out, int n_images, int C, void* stream) {
    if (n_images <= 0) return 0;
    return kcheck(launch_patch_embed(pix, wt, bias, pos, out, n_images, C, 1024, (hipStream_t)stream));
}

extern "C" int saber_k_perm_index(int y, int x, int stage) { return perm_index(y, x, stage); }

extern "C" int saber_k_dec_i2t(const uint16_t* X, int64_t x_batch_stride, const uint16_t* peq, const uint16_t* Kt, const float* tk, float kscale, const float* cb,
                               const uint16_t* VtT, const float* bo, const float* gamma, const float* beta, float eps, uint16_t* Xout, int P,
                               void* stream) {
    return kcheck(launch_dec_i2t(X, XMap{x_batch_stride, 1, 0}, peq, Kt, tk, kscale, cb, VtT, bo, gamma, beta, eps, Xout, P, (hipStream_t)stream));
}

extern "C" int saber_k_dec_i2t16(const uint16_t* X, int64_t x_batch_stride, const uint16_t* peq, const uint16_t* Kt, const float* tk, float kscale, const float* cb,
                                 const uint16_t* VtT, const float* bo, const float* gamma, const float* beta, float eps, uint16_t* Xout, int P, int nvalid,
                                 void* stream) {
    return kcheck(launch_dec_i2t16(X, XMap{x_batch_stride, 1, 0}, peq, Kt, tk, kscale, cb, VtT, bo, gamma, beta, eps, Xout, P, nvalid, (hipStream_t)stream));
}

extern "C" int saber_k_dec_t2i(const uint16_t* X, int64_t x_batch_stride, const uint16_t* pek, const uint16_t* Qt, const float* tq, float qscale, float* part_ws,
                               float* ml_ws, int P, int split, const uint16_t* Wv, const float* bv, uint16_t* out, void* stream) {
    return kcheck(launch_dec_t2i(X, XMap{x_batch_stride, 1, 0}, pek, Qt, tq, qscale, part_ws, ml_ws, P, split, Wv, bv, out, (hipStream_t)stream));
}

// ------------------------------------------------------------------------------------------------ head of the mask decoder
// The ConvTranspose weights arrive in checkpoint layout and go through the packer saber_engine_finalize uses (saber_pack_upscale, engine.hip).
// They are packed once per call into one device temporary that is released after the launch has completed: the call returns with the
// stream drained (no scratch kept per thread or per device).  fp32 hyper goes through launch_hyper_pack into the same temporary (the kernel reads
// the packed hi / lo operand, as in the engine); no counter: `sentinel` counts the stored logits alone.
extern "C" int saber_k_dec_upscale(const uint16_t* X, const float* w0, const float* b0, const float* ln_gamma, const float* ln_beta, const float* w3, const float* b3,
                                   const float* fs1, const float* fs0, int slot_div, int slot_off, const float* hyper, float* masks4, int P, const uint8_t* live,
                                   const float* iou4, int multimask, unsigned int* sentinel, void* stream) {
    if (P <= 0) return 0;
    if (!X || !w0 || !b0 || !ln_gamma || !ln_beta || !w3 || !b3 || !fs1 || !fs0 || !hyper || !masks4) return kfail("dec_upscale: null pointer");
    if (slot_div <= 0 || slot_off < 0) return kfail("dec_upscale: slot_div must be positive and slot_off non-negative");
    hipStream_t s = (hipStream_t)stream;
    const bool f16 = saber_op_is_f16();
    // checkpoint tensors -> host (hipMemcpyDefault: device or host pointers)
    std::vector<float> hw0((size_t)256 * 64 * 4), hb0(64), hw3((size_t)64 * 32 * 4), hb3(32);
    hipError_t st = hipMemcpyAsync(hw0.data(), w0, hw0.size() * 4, hipMemcpyDefault, s);
    if (st == hipSuccess) st = hipMemcpyAsync(hb0.data(), b0, hb0.size() * 4, hipMemcpyDefault, s);
    if (st == hipSuccess) st = hipMemcpyAsync(hw3.data(), w3, hw3.size() * 4, hipMemcpyDefault, s);
    if (st == hipSuccess) st = hipMemcpyAsync(hb3.data(), b3, hb3.size() * 4, hipMemcpyDefault, s);
    if (st == hipSuccess) st = hipStreamSynchronize(s);
    if (st != hipSuccess) return kfail(hipGetErrorString(st));
    UpscalePack up;
    saber_pack_upscale(hw0.data(), hb0.data(), hw3.data(), hb3.data(), &up);
    // one temporary: W1 [256][256] | W2p [128][64] (16-bit operand type) | b1 [256] | b2 [128] (fp32) | hyper_pk [P][256] (16-bit operand type)
    const size_t n1 = up.w1.size(), n2 = up.w2p.size(), w_bytes = (n1 + n2) * sizeof(bf16_t);
    std::vector<unsigned char> host(w_bytes + (up.b1.size() + up.b2.size()) * 4);
    bf16_t* hw = reinterpret_cast<bf16_t*>(host.data());
    for (size_t i = 0; i < n1 + n2; ++i) {
        const float v = i < n1 ? up.w1[i] : up.w2p[i - n1];
        if (f16 && !(std::fabs(v) <= 65504.0f)) return kfail("dec_upscale: a weight exceeds the fp16 range (65504)");      // as saber_engine_finalize refuses it
        hw[i] = saber_host_f2op(v, f16);
    }
    memcpy(host.data() + w_bytes, up.b1.data(), up.b1.size() * 4);
    memcpy(host.data() + w_bytes + up.b1.size() * 4, up.b2.data(), up.b2.size() * 4);
    unsigned char* dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&dev), host.size() + (size_t)P * 256 * sizeof(bf16_t)) != hipSuccess) return kfail("dec_upscale: allocation of the packed weights failed");
    int rc = 0;
    st = hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, s);
    if (st != hipSuccess) rc = kfail(hipGetErrorString(st));
    if (rc == 0) {
        const bf16_t* W1 = reinterpret_cast<const bf16_t*>(dev);
        const float* b1 = reinterpret_cast<const float*>(dev + w_bytes);
        bf16_t* hyper_pk = reinterpret_cast<bf16_t*>(dev + host.size());      // (a multiple of 16 bytes; the launchers check the alignment)
        rc = kcheck(launch_hyper_pack(hyper, P, hyper_pk, nullptr, s));
        if (rc == 0)
            rc = kcheck(launch_dec_upscale(X, W1, b1, ln_gamma, ln_beta, W1 + n1, b1 + up.b1.size(), fs1, fs0, XMap{0, slot_div, slot_off}, hyper, hyper_pk, masks4, P, s, live,
                                           iou4, multimask, sentinel));
    }
    st = hipStreamSynchronize(s);          // the launch has completed (and the upload has left `host`) before either temporary goes
    (void)hipFree(dev);
    if (rc == 0 && st != hipSuccess) rc = kfail(hipGetErrorString(st));
    return rc;
}
extern "C" int saber_k_hyper_pack(const float* hyper, int P, uint16_t* out, unsigned int* nonfinite_counter, void* stream) {
    if (P > 0 && (!hyper || !out)) return kfail("hyper_pack: null pointer");
    return kcheck(launch_hyper_pack(hyper, P, out, nonfinite_counter, (hipStream_t)stream));
}
extern "C" int saber_k_mask_pick(const float* masks4, const float* iou4, int P, int multimask, float* out_iou, int* out_sel, const uint8_t* live, void* stream) {
    if (P > 0 && (!iou4 || !out_iou || (!multimask && !masks4))) return kfail("mask_pick: null pointer");
    return kcheck(launch_mask_pick(masks4, iou4, P, multimask, out_iou, out_sel, (hipStream_t)stream, live));
}
extern "C" int saber_k_mask_select(const float* masks4, const float* iou4, int P, int multimask, float* out_masks, float* out_iou, void* stream) {
    if (P > 0 && (!masks4 || !iou4 || !out_masks || !out_iou)) return kfail("mask_select: null pointer");
    // counts_ws: the engine passes its [2 P] workspace; neither form of the kernel reads it (the dynamic form counts in its own block, the
    // multimask form copies planes 1-3), so none is allocated here
    return kcheck(launch_mask_select(masks4, iou4, P, multimask, out_masks, out_iou, nullptr, (hipStream_t)stream));
}
extern "C" int saber_k_iou_live_flags(const float* iou4, int P, float thr, uint8_t* live, unsigned long long* counters, void* stream) {
    if (P > 0 && (!iou4 || !live)) return kfail("iou_live_flags: null pointer");
    return kcheck(launch_iou_live_flags(iou4, P, thr, live, counters, (hipStream_t)stream));
}

int g_saber_debug_flags = 0;
unsigned long long* g_saber_stamp_buf = nullptr;   // development: device buffer for in-kernel cycle stamps (nullptr in production)
extern "C" void saber_k_set_stamp_buffer(void* dev) { g_saber_stamp_buf = (unsigned long long*)dev; }
extern "C" void saber_k_set_debug(int flags) { g_saber_debug_flags = flags; }
// 16-bit operand type of the kernel-level entry points called from THIS thread: 0 = bf16 (default), 1 = fp16 (common.h "OPERAND TYPE").
// The engine-level C-ABI sets it per call from the handle's precision mode and restores it on return (DeviceGuard, engine.h).
thread_local int g_saber_op_f16 = 0;
bf16_t saber_host_f2h(float f);          // engine.hip
// host-side fp32 -> IEEE half conversion the engine converts its weights with (exposed for the CPU test against numpy.float16)
extern "C" void saber_k_host_f32_to_f16(const float* in, uint16_t* out, int64_t n) { for (int64_t i = 0; i < n; ++i) out[i] = saber_host_f2h(in[i]); }
// A HIP stream whose kernels run on the first n_cus compute units of `first_cu`.. (hipExtStreamCreateWithCUMask; bit i of the mask = CU i in
// the runtime's numbering, which interleaves the XCDs: consecutive indices are spread over all eight) - the co-residency experiment of
// VERDICT r03 item 4 (tools/cu_mask_bench.py).  The handle can be wrapped in torch.cuda.ExternalStream.
extern "C" int saber_k_stream_create_cu_range(int first_cu, int n_cus, void** out_stream) {
    if (!out_stream || first_cu < 0 || n_cus < 1 || first_cu + n_cus > 1024) return kfail("stream_create_cu_range: bad argument");
    uint32_t mask[32] = {0};
    for (int c = first_cu; c < first_cu + n_cus; ++c) mask[c >> 5] |= 1u << (c & 31);
    hipStream_t s = nullptr;
    const hipError_t st = hipExtStreamCreateWithCUMask(&s, (uint32_t)((first_cu + n_cus + 31) / 32), mask);
    if (st != hipSuccess) return kfail(hipGetErrorString(st));
    *out_stream = (void*)s;
    return 0;
}
extern "C" int saber_k_stream_destroy(void* stream) { return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? 0 : kfail("hipStreamDestroy failed"); }
int saber_cu_count() {
    static std::atomic<int> table[64];                      // zero-initialised; 0 = not queried yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = table[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    hipDeviceProp_t pr;
    n = (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
    table[dev].store(n, std::memory_order_relaxed);         // (every thread that races here computes the same value)
    return n;
}

extern "C" int saber_k_set_operand_type(int f16) { const int prev = g_saber_op_f16; g_saber_op_f16 = f16 ? 1 : 0; return prev; }

// ------------------------------------------------------------------------------------------------ video (memory) path kernels
extern "C" int saber_k_rope(const float* x, int64_t rows, int n_rot, int C, int side, float theta, float* out_f32, uint16_t* out_bf16, void* stream) {
    return kcheck(launch_rope(x, rows, n_rot, C, side, theta, out_f32, out_bf16, (hipStream_t)stream));
}
extern "C" int saber_k_softmax_rows(const float* S, int64_t ld_s, int64_t rows, int n, float scale, uint16_t* P, int64_t ld_p, void* stream) {
    return kcheck(launch_softmax_rows(S, ld_s, rows, n, scale, P, ld_p, (hipStream_t)stream));
}
extern "C" int saber_k_conv3x3s2(const float* in, int H, int W, int Cin, const float* w, const float* b, int Cout, float* out, void* stream) {
    return kcheck(launch_conv3x3s2(in, H, W, Cin, w, b, Cout, out, (hipStream_t)stream));
}
extern "C" int saber_k_conv3x3s2_t(const float* in, int H, int W, int Cin, const float* wt, const float* b, int Cout, float* out, void* stream) {
    return kcheck(launch_conv3x3s2_t(in, H, W, Cin, wt, b, Cout, out, (hipStream_t)stream));
}
extern "C" int saber_k_paint_nearest(const float* logits, int Hv, int Wv, float thr, int label, uint16_t* plane, int H, int W, int* any_flag, void* stream) {
    return kcheck(launch_paint_nearest(logits, Hv, Wv, thr, label, plane, H, W, any_flag, (hipStream_t)stream));
}
extern "C" int saber_k_unpack_masks(const uint32_t* bits, int n, int H, int W, uint8_t* out, void* stream) {
    if (n > 0 && (!bits || !out)) return kcheck("unpack_masks: null pointer");
    return kcheck(launch_unpack_masks(bits, n, H, W, out, (hipStream_t)stream));
}
extern "C" int saber_k_dwconv7(const float* in, int H, int W, int C, const float* w, const float* b, float* out, void* stream) {
    return kcheck(launch_dwconv7(in, H, W, C, w, b, out, (hipStream_t)stream));
}
extern "C" int saber_k_dwconv7_t(const float* in, int H, int W, int C, const float* wt, const float* b, float* out, void* stream) {
    return kcheck(launch_dwconv7_t(in, H, W, C, wt, b, out, (hipStream_t)stream));
}
extern "C" int saber_k_conv3x3s2_t_batched(const float* in, int64_t in_stride, int H, int W, int Cin, const float* wt, const float* b, int Cout, float* out,
                                           int64_t out_stride, int batch, void* stream) {
    return kcheck(launch_conv3x3s2_t_batched(in, in_stride, H, W, Cin, wt, b, Cout, out, out_stride, batch, (hipStream_t)stream));
}
extern "C" int saber_k_dwconv7_t_batched(const float* in, int64_t in_stride, int H, int W, int C, const float* wt, const float* b, float* out, int64_t out_stride,
                                         int batch, void* stream) {
    return kcheck(launch_dwconv7_t_batched(in, in_stride, H, W, C, wt, b, out, out_stride, batch, (hipStream_t)stream));
}
extern "C" int saber_k_conv4x4s4(const float* in, int H, int W, const float* w, const float* b, float* out, void* stream) {
    return kcheck(launch_conv4x4s4(in, H, W, w, b, out, (hipStream_t)stream));
}
extern "C" int saber_k_resize_plane(const float* in, int n_planes, int H, int W, float* out, int Ho, int Wo, int antialias, int post, float a, float c, void* stream) {
    return kcheck(launch_resize_plane(in, n_planes, H, W, out, Ho, Wo, antialias, post, a, c, (hipStream_t)stream));
}
extern "C" int saber_k_resize_planes_non_overlap(const float* in, int n_planes, int H, int W, float* out, int Ho, int Wo, float suppress_max, void* stream) {
    if (const char* m = launch_resize_planes_non_overlap(in, n_planes, H, W, out, Ho, Wo, suppress_max, (hipStream_t)stream)) return kfail(m);
    return n_planes == 0 ? 0 : kcheck(nullptr);
}
extern "C" int saber_k_gemm_mx(const uint8_t* A, int64_t lda, const uint8_t* SA, int64_t sa_rows, const uint8_t* W, int64_t ldw, const uint8_t* SW, int64_t sw_rows, const float* bias,
                               const float* res, float* out_f32, uint16_t* out_bf16, uint8_t* out_mx, uint8_t* out_mx_scales, int64_t out_mx_rows, int64_t ldc, int64_t M, int N, int Kp,
                               int act, void* stream) {
    GemmMxParams p;
    p.A = A; p.lda = lda; p.SA = SA; p.sa_rows = sa_rows; p.W = W; p.ldw = ldw; p.SW = SW; p.sw_rows = sw_rows; p.bias = bias;
    p.res = res; p.ldres = ldc; p.Cf = out_f32; p.ldcf = ldc; p.Cb = out_bf16; p.ldcb = ldc; p.C8 = out_mx; p.ldc8 = ldc; p.SC = out_mx_scales; p.sc_rows = out_mx_rows;
    p.M = M; p.N = N; p.Kp = Kp; p.act = act;
    return kcheck(launch_gemm_mx(p, (hipStream_t)stream));
}
extern "C" int saber_k_quant_mx(const uint16_t* x, int64_t ldx, int C, uint8_t* out, int64_t ldo, int Kp, uint8_t* scales, int64_t scale_rows, int64_t M, void* stream) {
    return kcheck(launch_quant_mx_bf16(x, ldx, C, out, ldo, Kp, scales, scale_rows, M, (hipStream_t)stream));
}
extern "C" int saber_k_ln_mx(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int C, uint8_t* out, int64_t ldo, int Kp, uint8_t* scales,
                             int64_t scale_rows, int64_t M, void* stream) {
    return kcheck(launch_ln_mx(x, ldx, gamma, beta, eps, C, out, ldo, Kp, scales, scale_rows, M, (hipStream_t)stream));
}
extern "C" int saber_k_box_nms(const float* boxes_xyxy, const float* scores, int n, float iou_thresh, void* scratch, int* keep_out, int* count_out, void* stream) {
    return kcheck(launch_box_nms_probe(boxes_xyxy, scores, n, iou_thresh, scratch, keep_out, count_out, (hipStream_t)stream));
}
extern "C" int saber_k_flash256(const uint16_t* Q, const uint16_t* K, const uint16_t* V, int n_q, int n_keys, float scale, const float* bias_v, uint16_t* out, float* ws,
                                int64_t ws_floats, void* stream) {
    return kcheck(launch_flash256(Q, K, V, n_q, n_keys, scale, bias_v, out, ws, (size_t)ws_floats, (hipStream_t)stream));
}
extern "C" int saber_k_gauss_mirror(const float* in, float* out, int n_planes, int H, int W, int axis, double sigma, void* stream) {
    return kcheck(launch_gauss_mirror(in, out, n_planes, H, W, axis, sigma, (hipStream_t)stream));
}
extern "C" int saber_k_axpy(const float* x, const float* y, const float* g, float alpha, int64_t rows, int C, float* out, void* stream) {
    return kcheck(launch_axpy(x, y, g, alpha, rows, C, out, (hipStream_t)stream));
}
// slab preparation (volprep.hip)
extern "C" int saber_k_correlate1d_zero(const void* in, int dtype, float* out, int64_t outer, int64_t len, int64_t inner, const float* taps_host, int ks,
                                        int chunk_len, float* minmax_dev, void* stream) {
    return kcheck(launch_correlate1d_zero(in, dtype, out, outer, len, inner, taps_host, ks, chunk_len, minmax_dev, (hipStream_t)stream));
}
extern "C" int saber_k_normalize_minmax(float* v, int64_t n, const float* minmax_dev, void* stream) {
    return kcheck(launch_normalize_minmax(v, n, minmax_dev, (hipStream_t)stream));
}
extern "C" int saber_k_project_mean(const float* vol, int Z, int H, int W, int z0, int z1, float* out, void* stream) {
    return kcheck(launch_project_mean(vol, Z, H, W, z0, z1, out, (hipStream_t)stream));
}
// propagated label volumes (labelvol.hip)
extern "C" int saber_k_paint_nearest_stack(const float* logits, int n, int Hv, int Wv, const int* labels_host, float thr, uint16_t* plane, int H, int W,
                                           int* any_flag, void* stream) {
    return kcheck(launch_paint_nearest_stack(logits, n, Hv, Wv, labels_host, thr, plane, H, W, any_flag, (hipStream_t)stream));
}
extern "C" int saber_k_relabel_frames(uint16_t* vol, int Z, int64_t HW, const uint16_t* lut, int L, void* stream) {
    return kcheck(launch_relabel_frames(vol, Z, HW, lut, L, (hipStream_t)stream));
}
extern "C" int saber_k_merge_max_u16(uint16_t* acc, const uint16_t* src, int64_t n, int binarize, void* stream) {
    return kcheck(launch_merge_max_u16(acc, src, n, binarize, (hipStream_t)stream));
}
extern "C" int saber_k_merge_class_conf(uint16_t* final_labels, float* best, const uint16_t* src, const uint16_t* cls, const float* conf, int L, int64_t n,
                                        void* stream) {
    return kcheck(launch_merge_class_conf(final_labels, best, src, cls, conf, L, n, (hipStream_t)stream));
}
// hole filling of mask logits (holefill.hip)
extern "C" int saber_k_fill_holes(const float* in, int n_planes, int H, int W, int max_area, float fill_value, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return kcheck(launch_fill_holes(in, n_planes, H, W, max_area, fill_value, out, workspace, workspace_bytes, (hipStream_t)stream));
}
// small holes filled and small islands removed on bit-packed masks (smallregions.hip)
extern "C" int saber_k_mask_small_regions(const uint32_t* bits_in, int n, int H, int W, int min_area, uint32_t* bits_out, int32_t* changed, int32_t* area,
                                          int32_t* box_xyxy, void* workspace, size_t workspace_bytes, void* stream) {
    return kcheck(launch_small_regions(bits_in, n, H, W, min_area, bits_out, changed, area, box_xyxy, workspace, workspace_bytes, (hipStream_t)stream));
}
extern "C" size_t saber_k_mask_small_regions_bytes(int H, int W) { return small_regions_bytes_per_mask(H, W); }
// small holes and sprinkles of low-resolution logit planes, in place (lowres_cleanup.hip)
extern "C" int saber_k_clean_lowres(float* planes, const int* idx, const uint8_t* pass, int n, int H, int W, float thr, int max_hole_area, int max_sprinkle_area,
                                    void* stream) {
    return kcheck(launch_clean_lowres(planes, idx, pass, n, H, W, thr, max_hole_area, max_sprinkle_area, (hipStream_t)stream));
}
// run lengths of bit-packed masks, upstream's uncompressed RLE (rle.hip)
extern "C" size_t saber_k_rle_workspace_bytes(int n, int H, int W) { return rle_workspace_bytes(n, H, W); }
extern "C" int saber_k_rle_count(const uint32_t* bits, int n, int H, int W, int64_t* offsets, void* ws, size_t ws_bytes, void* stream) {
    return kcheck(launch_rle_count(bits, n, H, W, offsets, ws, ws_bytes, (hipStream_t)stream));
}
extern "C" int saber_k_rle_encode(const uint32_t* bits, int n, int H, int W, const int64_t* offsets, uint32_t* counts, int64_t capacity, void* ws, size_t ws_bytes,
                                  void* stream) {
    return kcheck(launch_rle_encode(bits, n, H, W, offsets, counts, capacity, ws, ws_bytes, (hipStream_t)stream));
}
extern "C" int saber_k_rle_decode(const uint32_t* counts, const int64_t* offsets, int n, int H, int W, uint32_t* bits_out, void* stream) {
    return kcheck(launch_rle_decode(counts, offsets, n, H, W, bits_out, (hipStream_t)stream));
}
// window-sized bit-packed masks -> full-frame rows / label stack (windows.hip)
extern "C" int saber_k_place_window_masks(const uint32_t* src, const saber_window_mask* table_dev, int n, int H, int W, uint32_t* out, void* stream) {
    return kcheck(launch_window_place(src, table_dev, n, H, W, out, (hipStream_t)stream));
}
extern "C" int saber_k_window_label_stack(const uint32_t* src, const saber_window_mask* table_dev, int first, int count, int H, int W, int elem_bytes, void* out,
                                          void* stream) {
    return kcheck(launch_window_stack(src, table_dev, first, count, H, W, elem_bytes, out, (hipStream_t)stream));
}
extern "C" int saber_k_add_to_bf16(const float* x, const float* y, int y_rows, uint16_t* out_bf16, float* out_f32, int64_t rows, int C, void* stream) {
    return kcheck(launch_add_to_bf16(x, y, y_rows, out_bf16, out_f32, rows, C, (hipStream_t)stream));
}
// batched GEMM with explicit strides (scores / values of the memory attention, one batch entry per tracked object)
extern "C" int saber_k_gemm_batched(const uint16_t* A, int lda, int64_t strideA, const uint16_t* W, int ldw, int64_t strideW, const float* bias, float* out_f32,
                                    int ldcf, int64_t strideCf, uint16_t* out_bf16, int ldcb, int64_t strideCb, int M, int N, int K, int batch, void* stream) {
    GemmParams p;
    p.A = A; p.lda = lda; p.strideA = strideA; p.W = W; p.ldw = ldw; p.strideW = strideW; p.bias = bias; p.Cf = out_f32; p.ldcf = ldcf; p.strideCf = strideCf;
    p.Cb = out_bf16; p.ldcb = ldcb; p.strideCb = strideCb; p.M = M; p.N = N; p.K = K; p.batch = batch;
    return kcheck(launch_gemm(p, (hipStream_t)stream));
}
extern "C" int saber_k_bf16_to_f32(const uint16_t* x, int64_t n, float* out, void* stream) { return kcheck(launch_bf16_to_f32(x, n, out, (hipStream_t)stream)); }
// ---- memory attention of all tracked objects of a frame (flash256.hip, video_ops.hip, gemm.hip's batch dimension)
extern "C" int saber_k_flash256_batched(const uint16_t* Q, int64_t q_stride, const uint16_t* K, int64_t k_stride, const uint16_t* V, int64_t v_stride, int n_q, int n_keys,
                                        int batch, float scale, const float* bias_v, uint16_t* out, int64_t o_stride, float* ws, int64_t ws_floats, void* stream) {
    if (ws_floats < 0) return kfail("flash256_batched: ws_floats must be non-negative");
    return kcheck(launch_flash256_batched(Q, q_stride, K, k_stride, V, v_stride, n_q, n_keys, batch, scale, bias_v, out, o_stride, ws, (size_t)ws_floats, (hipStream_t)stream));
}
extern "C" int saber_k_rope_batched(const float* x, int64_t rows_per, int batch, int n_rot, int C, int side, float theta, float* out_f32, uint16_t* out_bf16, void* stream) {
    return kcheck(launch_rope_batched(x, rows_per, batch, n_rot, C, side, theta, out_f32, out_bf16, (hipStream_t)stream));
}
extern "C" int saber_k_membank_assemble(const void* const* mem_ptrs, const int* pos_idx, int n_mem, const float* pos_tables, int n_tables, const uint16_t* ptr_tok,
                                        int64_t ptr_tok_stride, const float* ptr_pos, int64_t ptr_pos_stride, int n_ptr_rows, int batch, uint16_t* mem_out,
                                        uint16_t* kin_out, void* stream) {
    return kcheck(launch_membank_assemble(reinterpret_cast<const bf16_t* const*>(mem_ptrs), pos_idx, n_mem, pos_tables, n_tables, ptr_tok, ptr_tok_stride, ptr_pos,
                                          ptr_pos_stride, n_ptr_rows, batch, mem_out, kin_out, (hipStream_t)stream));
}
extern "C" int saber_k_gemm_ld_batched(const uint16_t* A, int lda, int64_t strideA, const uint16_t* W, int ldw, int w_kpad, const float* bias, const float* res,
                                       int64_t strideRes, float* out_f32, int64_t strideCf, uint16_t* out_bf16, int64_t strideCb, int M, int N, int K, int act, int batch,
                                       void* stream) {
    if (batch < 1 || batch > 65535) return kfail("gemm_ld_batched: batch must be in 1..65535");
    if (strideA < 0 || strideRes < 0 || (batch > 1 && ((out_f32 && strideCf < (int64_t)M * N) || (out_bf16 && strideCb < (int64_t)M * N))))
        return kfail("gemm_ld_batched: bad stride (outputs must not overlap)");
    // saber_k_gemm_ld's packed-W route (persistent 256 x 256 tiles) has no batch dimension: its summation order cannot be reproduced here
    if (w_kpad && out_bf16 && !out_f32 && !res && (K % 64) == 0 && (N & 7) == 0 && ((int64_t)M * N >= (int64_t)1024 * 65536 || (g_saber_debug_flags & 128)))
        return kfail("gemm_ld_batched: this shape takes saber_k_gemm_ld's packed-W route, which has no batch dimension");
    GemmParams p;
    p.A = A; p.lda = lda; p.strideA = strideA; p.W = W; p.ldw = ldw; p.bias = bias; p.res = res; p.ldres = N; p.strideRes = strideRes;
    p.Cf = out_f32; p.ldcf = N; p.strideCf = strideCf; p.Cb = out_bf16; p.ldcb = N; p.strideCb = strideCb;
    p.M = M; p.N = N; p.K = K; p.act = act; p.w_kpad = w_kpad; p.batch = batch;
    return kcheck(launch_gemm(p, (hipStream_t)stream));
}

// ------------------------------------------------------------------------------------------------ exact-precision (fp32) kernels (exact.hip)
// The launchers the engine's exact mode calls, as they stand; the checks here only keep divisors and the batch count positive.
extern "C" int saber_k_xg_gemm(const float* A, int64_t lda, int64_t sA, const float* A2, int64_t lda2, int64_t a2_mod, const float* W, int64_t ldw, int64_t sW,
                               const float* bias, int64_t sBias, const float* res, int64_t ldres, int res_shift, int64_t res_mod, int64_t res_rows_per,
                               int64_t res_stride, int res_div, int res_off, float* C, int64_t ldc, int64_t sC, int M, int N, int K, int act, int act_last,
                               int pool4, int batch, void* stream) {
    if (batch < 1) return kfail("xg_gemm: batch must be positive");
    if (A2 && a2_mod < 1) return kfail("xg_gemm: a2_mod must be positive");
    if (res && res_rows_per > 0 && (res_div < 1 || res_off < 0)) return kfail("xg_gemm: res_div must be positive and res_off non-negative");
    if (res && (res_mod < 0 || res_shift < 0 || res_shift > 31)) return kfail("xg_gemm: bad residual mapping");
    XGemm p;
    p.A = A; p.lda = lda; p.sA = sA; p.A2 = A2; p.lda2 = lda2; p.a2_mod = a2_mod; p.W = W; p.ldw = ldw; p.sW = sW; p.bias = bias; p.sBias = sBias;
    p.res = res; p.ldres = ldres; p.res_shift = res_shift; p.res_mod = res_mod; p.res_rows_per = res_rows_per; p.res_stride = res_stride; p.res_div = res_div;
    p.res_off = res_off; p.C = C; p.ldc = ldc; p.sC = sC; p.M = M; p.N = N; p.K = K; p.act = act; p.act_last = act_last; p.pool4 = pool4; p.batch = batch;
    return kcheck(xg_gemm(p, (hipStream_t)stream));
}
extern "C" int saber_k_xg_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out, int64_t rows, int C, int act,
                                    const uint8_t* row_valid, int valid_mod, void* stream) {
    if (C < 1) return kfail("xg_layernorm: C must be positive");
    if (row_valid && valid_mod < 1) return kfail("xg_layernorm: valid_mod must be positive");
    return kcheck(xg_layernorm(x, LnW{gamma, beta}, eps, out, rows, C, act, (hipStream_t)stream, row_valid, valid_mod));
}
extern "C" int saber_k_xg_attention(int hd, const float* q, int64_t q_bs, int ldq, const float* k, int64_t k_bs, int ldk, const float* v, int64_t v_bs, int ldv,
                                    float* o, int64_t o_bs, int ldo, int nq, int nk, int batch, int heads, int qpool, const uint8_t* kmask, float scale,
                                    void* stream) {
    if (nk < 1 || heads < 1) return kfail("xg_attention: nk and heads must be positive");
    return kcheck(xg_attn(hd, q, q_bs, ldq, k, k_bs, ldk, v, v_bs, ldv, o, o_bs, ldo, nq, nk, batch, heads, qpool, kmask, scale, (hipStream_t)stream));
}
extern "C" int saber_k_xg_add(const float* x, const float* y, int64_t ymod, float* out, int64_t rows, int C, void* stream) {
    if (C < 1 || ymod < 0) return kfail("xg_add: C must be positive and ymod non-negative");
    xg_add(x, y, ymod, out, rows, C, (hipStream_t)stream);
    return kcheck(nullptr);
}
extern "C" int saber_k_xg_add_slot(const float* in, const float* tab, int64_t stride, int div, int off, const float* vec, float* out, int64_t rows_per, int C,
                                   int P, int act, void* stream) {
    if (C < 1 || div < 1 || off < 0) return kfail("xg_add_slot: C and div must be positive and off non-negative");
    xg_add_slot(in, tab, XMap{stride, div, off}, vec, out, rows_per, C, P, act, (hipStream_t)stream);
    return kcheck(nullptr);
}
extern "C" int saber_k_xg_mask_hidden(const float* mask_in, int P, const float* w1, const float* b1, const float* g1, const float* be1, const float* w2,
                                      const float* b2, const float* g2, const float* be2, float clamp_abs, int raw4_q0, float* out, void* stream) {
    const MaskEmbedWeights w{w1, b1, g1, be1, w2, b2, g2, be2, nullptr, nullptr};
    xg_mask_hidden(mask_in, P, w, clamp_abs, raw4_q0, out, (hipStream_t)stream);
    return kcheck(nullptr);
}
extern "C" int saber_k_xg_mask_dot(const float* up, const float* hyper, int P, float* masks4, void* stream) {
    xg_mask_dot(up, hyper, P, masks4, (hipStream_t)stream);
    return kcheck(nullptr);
}
