// The C API of the kernel library (_C_hip.so): the one declaration of every exported `pa_*` launcher.
//
// common.h includes this header, so every csrc/kernels/*.hip sees the declaration of what it defines and a
// definition whose parameters or return type differ fails to compile ("conflicting types for 'pa_...'"). The C++
// callers (csrc/interpreter/*.cpp, csrc/dispatch/dispatch.cpp) include it instead of declaring launchers of their
// own, and the ctypes view (paddlepaddle_amd/ops/_sigs.py) is checked against it when _C_dispatch is built.
// A new launcher is declared here, under its file, with the parameter list of its definition.
//
// Host-only and plain: no device code, compiles with hipcc and with g++ -D__HIP_PLATFORM_AMD__=1.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#define PA_EXPORT extern "C" __attribute__((visibility("default")))

// Optional arguments of the flash-attention launchers (mirrored by paddlepaddle_amd/ops/attention.py:_AttnExtra,
// all 8-byte fields).
struct PaAttnExtra {
  const int* cu_q; const int* cu_k;
  const void* mask; int64_t mask_kind; int64_t ms[3];
  const int* fm; int64_t fm_cols; int64_t fms[2];
  const int* fm_stats; int64_t fmst[2];
  double drop_p; uint64_t seed;
  int64_t lse_s[2];  // 0, 0 -> dense [B, H, Sq]
  int64_t dtype;     // 0 bf16, 1 fp16
};

// act.hip
PA_EXPORT int pa_gelu_fwd(const void* x, void* y, int64_t n, int approx, int dtype, hipStream_t st);
PA_EXPORT int pa_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int approx, int dtype, hipStream_t st);
PA_EXPORT int pa_bias_gelu_fwd(const void* x, const void* b, void* y, int64_t rows, int64_t cols, int dtype,
                               hipStream_t st);
PA_EXPORT int pa_swiglu_fwd(const void* a, const void* b, void* y, int64_t rows, int64_t cols, int64_t ld, int dtype,
                            hipStream_t st);
PA_EXPORT int pa_swiglu_bwd(const void* a, const void* b, const void* dy, void* da, void* db, int64_t rows,
                            int64_t cols, int64_t ld_packed, int dtype, hipStream_t st);
PA_EXPORT int pa_rope_fwd(const void* x, const float* cs, const float* sn, void* out, int64_t B, int64_t S, int64_t H,
                          int64_t D, int flags, int dtype, hipStream_t st);
PA_EXPORT int pa_rope_rows(const void* x, int64_t ldx, const float* cs, const float* sn, void* out, int64_t ldo,
                           int64_t rows, int64_t S, int64_t NH, int64_t D, int flags, int dtype, hipStream_t st);

// adamw.hip
PA_EXPORT int64_t pa_multi_tensor_chunk();
PA_EXPORT int pa_adamw_multi(const int64_t* table, const int64_t* items, int64_t n_items, const float* inv_scale,
                             float lr, float b1, float b2, float eps, float wd_unused, float bc1, float bc2,
                             const float* hyper, hipStream_t st);
PA_EXPORT int pa_adam_hyper_step(float* hyper, float b1, float b2, hipStream_t st);
PA_EXPORT int pa_sq_norm_multi(const int64_t* table, const int64_t* items, int64_t n_items, float* partial,
                               hipStream_t st);
PA_EXPORT int pa_momentum_multi(const int64_t* table, const int64_t* items, int64_t n_items, const float* inv_scale,
                                float lr, float mu, float rescale, int nesterov, hipStream_t st);
PA_EXPORT int pa_write_i64(int64_t* dst, const int64_t* src, int64_t n, hipStream_t st);

// amp.hip
PA_EXPORT int pa_amp_check_unscale_multi(const int64_t* table, const int64_t* items, int64_t n_items,
                                         const float* inv_scale, float* found_inf, hipStream_t st);

// bn.hip
PA_EXPORT int pa_bn_set_target_wgs(int n);
PA_EXPORT int pa_bn_chunks(int64_t R, int C);
PA_EXPORT int pa_bn_fwd_nhwc(const void* x, const void* res, void* y, const float* w, const float* b, float* run_mean,
                             float* run_var, float* save_mean, float* save_rstd, float* partial, float* ss, int64_t R,
                             int C, float momentum, float eps, int relu, int training, hipStream_t st);
PA_EXPORT int pa_bn_bwd_nhwc(const void* dy, const void* x, const void* y, void* dx, void* dres, const float* w,
                             const float* mean, const float* rstd, float* dw, float* db, float* partial, float* coef,
                             int64_t R, int C, int relu, int global_stats, const float* ss, hipStream_t st);
PA_EXPORT int pa_bn_fwd_nhwc_mask(const void* x, const void* res, void* y, const float* w, const float* b,
                                  float* run_mean, float* run_var, float* save_mean, float* save_rstd, float* partial,
                                  float* ss, void* mbits, int64_t R, int C, float momentum, float eps, int training,
                                  hipStream_t st);
PA_EXPORT int pa_bn_bwd_nhwc_mask(const void* dy, const void* x, const void* mbits, void* dx, void* dres,
                                  const float* w, const float* mean, const float* rstd, float* dw, float* db,
                                  float* partial, float* coef, int64_t R, int C, int global_stats, hipStream_t st);
PA_EXPORT int64_t pa_bn_pre_ws(int chunks, int C);
PA_EXPORT int pa_bn_fwd_nhwc_pre(const void* x, const void* res, void* y, const float* w, const float* b,
                                 float* run_mean, float* run_var, float* save_mean, float* save_rstd,
                                 const float* stats, int chunks, float* ws, float* ss, void* mbits, int64_t R, int C,
                                 float momentum, float eps, int relu, hipStream_t st);
PA_EXPORT int pa_bn_bwd_nhwc_pre(const void* dy, const void* x, void* dx, const float* w, const float* mean,
                                 const float* rstd, float* dw, float* db, const float* stats, int chunks, float* ws,
                                 float* coef, int64_t R, int C, int global_stats, const float* ss, hipStream_t st);
PA_EXPORT int pa_bn_reduce_nhwc(int mode, const void* x, const void* dy, const void* y, const float* mean,
                                const float* ss, float* partial, float* sums, int64_t R, int C, int relu,
                                hipStream_t st);
PA_EXPORT int pa_bn_bwd_apply_nhwc(const void* dy, const void* x, const void* y, const float* coef, void* dx,
                                   void* dres, int64_t R, int C, int relu, const float* ss, hipStream_t st);

// decode_attn.hip
PA_EXPORT int pa_paged_decode_attn(const void* q, const void* kc, const void* vc, const int* tables, const int* lens,
                                   float* part_o, float* part_ml, void* out, int N, int H, int Hkv, int D, int bs,
                                   int max_blocks, int splits, int64_t blk_stride, int64_t head_stride, float scale,
                                   hipStream_t st);
PA_EXPORT int pa_paged_decode_attn_q8(const void* q, const void* kc, const void* vc, const float* k_dq,
                                      const float* v_dq, const void* k_cur, const void* v_cur, const int* tables,
                                      const int* lens, float* part_o, float* part_ml, void* out, int N, int H,
                                      int Hkv, int D, int bs, int max_blocks, int splits, int64_t blk_stride,
                                      int64_t head_stride, float scale, hipStream_t st);

// decode_fused.hip
PA_EXPORT int pa_add_rms_norm_fwd(const void* x, const void* r, const void* w, void* s_out, void* y, int64_t rows,
                                  int64_t cols, float eps, int dtype, hipStream_t st);
PA_EXPORT int pa_decode_rope_cache(const void* qkv, int64_t ld, const float* cs, const float* sn, const int64_t* pos,
                                   void* q_out, void* kc, void* vc, int B, int H, int Hkv, int D, int64_t Lc,
                                   int dtype, hipStream_t st);
PA_EXPORT int pa_decode_rope_cache_q8(const void* qkv, int64_t ld, const float* cs, const float* sn,
                                      const int64_t* pos, void* q_out, void* kc, void* vc, const float* k_q,
                                      const float* v_q, int B, int H, int Hkv, int D, int64_t Lc, int dtype,
                                      hipStream_t st);

// dwconv.hip
PA_EXPORT int pa_dwconv_fwd(const void* x, const void* wt, const void* bias, void* y, const int* shape, int dtype,
                            hipStream_t st);
PA_EXPORT int pa_dwconv_dgrad(const void* dy, const void* wt, const void* x, void* dx, const int* shape, int dtype,
                              hipStream_t st);
PA_EXPORT int pa_dwconv_wgrad_parts(const int* shape, int* out /* nparts, stripes, CGB, ppl */);
PA_EXPORT int pa_dwconv_wgrad(const void* x, const void* dy, float* part, const int* shape, int dtype,
                              hipStream_t st);

// flash_attn.hip
PA_EXPORT int pa_flash_attn_set_fwd_variant(int v);
PA_EXPORT int pa_flash_attn_fwd_ex(const void* q, const void* k, const void* v, void* o, float* lse,
                                   const int64_t* strides, int B, int Sq, int Sk, int H, int Hk, int D, float scale,
                                   int causal, const PaAttnExtra* ex, hipStream_t st);
PA_EXPORT int pa_flash_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                                const int64_t* strides, int B, int Sq, int Sk, int H, int Hk, int D, float scale,
                                int causal, hipStream_t st);
PA_EXPORT int pa_flash_attn_bwd_ds_ok(int D, int has_mask, int has_fm, int dropout, int varlen);
PA_EXPORT int pa_flash_attn_bwd_ex(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                   const float* lse, void* dq, void* dk, void* dv, float* dq_acc, float* delta,
                                   const int64_t* strides, int B, int Sq, int Sk, int H, int Hk, int D, float scale,
                                   int causal, int64_t q_rows, const PaAttnExtra* ex, hipStream_t st);
PA_EXPORT int64_t pa_flash_attn_bwd_ds_bytes(int B, int Sq, int Sk, int H);
PA_EXPORT int pa_flash_attn_bwd_ds(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                   const float* lse, void* dq, void* dk, void* dv, void* ds, float* delta,
                                   const int64_t* strides, int B, int Sq, int Sk, int H, int Hk, int D, float scale,
                                   int causal, const PaAttnExtra* ex, hipStream_t st);
PA_EXPORT int pa_flash_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                const float* lse, void* dq, void* dk, void* dv, float* dq_acc, float* delta,
                                const int64_t* strides, int B, int Sq, int Sk, int H, int Hk, int D, float scale,
                                int causal, hipStream_t st);
PA_EXPORT int pa_fa_fm_stats(const int* fm, int cols, int causal, int Sk, int Bm, int Hm, int64_t sb, int64_t sh,
                             int ntiles, int* stats, hipStream_t st);

// gemm.hip
PA_EXPORT int64_t pa_gemm_pp_ws_bytes(int64_t M, int64_t N, int64_t K);
PA_EXPORT int pa_gemm_bf16_pp(const void* a, const void* b, void* c, const void* bias, void* aux, int64_t M,
                              int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor,
                              int flags, float alpha, void* ws, hipStream_t st);
PA_EXPORT int64_t pa_gemm_pp_splitk_ws_bytes(int64_t M, int64_t N, int splits);
PA_EXPORT int pa_gemm_bf16_pp_splitk(const void* a, const void* b, void* c, int64_t M, int64_t N, int64_t K,
                                     int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor, int flags,
                                     float alpha, int splits, void* ws, hipStream_t st);
PA_EXPORT int pa_gemm_bf16_pp_segs(const int64_t* seg, int nseg, int seg_k, const void* a, const void* b, void* c,
                                   const void* bias, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                   int64_t ldc, int a_kmajor, int b_kmajor, int flags, float alpha, void* ws,
                                   hipStream_t st);
PA_EXPORT int pa_gemm_bf16_4w(const void* a, const void* b, void* c, const void* bias, void* aux, int64_t M,
                              int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor,
                              int flags, float alpha, void* ws, hipStream_t st);
PA_EXPORT int pa_gemm_bf16_res(const void* a, const void* b, void* c, const void* bias, const void* res, int64_t M,
                               int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor,
                               int b_kmajor, void* ws, hipStream_t st);
PA_EXPORT int pa_gemm_bf16_dgelu(const void* a, const void* b, void* dh, const void* pre, float* colsum, int64_t M,
                                 int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor,
                                 int b_kmajor, int kern, hipStream_t st);
PA_EXPORT int pa_gemm_bf16_4w_abl(const void* a, const void* b, void* c, int64_t M, int64_t N, int64_t K, int abl,
                                  hipStream_t st);
PA_EXPORT int pa_gemm_bf16(const void* a, const void* b, void* c, const void* bias, void* aux, int64_t M, int64_t N,
                           int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor, int flags,
                           float alpha, int bn, int splits, hipStream_t st);
PA_EXPORT int pa_conv3d_ndhwc_fwd(const void* x, const void* w, const void* bias, void* out, const void* zero, int N,
                                  int D, int H, int W, int C, int Cout, int KD, int KH, int KW, int stride, int pad_d,
                                  int pad_h, int pad_w, int dil, int Do, int Ho, int Wo, hipStream_t st);
PA_EXPORT int pa_gemm_stats_chunks(int64_t M, int bn);
PA_EXPORT int pa_gemm_bf16_stats(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N,
                                 int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor,
                                 int flags, int bn, float* stats, hipStream_t st);
PA_EXPORT int pa_gemm_bf16_bnbwd(const void* a, const void* b, void* c, int64_t M, int64_t N, int64_t K, int64_t lda,
                                 int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor, int bn, const void* bn_x,
                                 const float* bn_ss, const float* bn_mean, float* stats, hipStream_t st);
PA_EXPORT int pa_conv2d_nhwc_fwd(const void* x, const void* w, const void* bias, void* out, const void* zero, int N,
                                 int H, int W, int C, int Cout, int KH, int KW, int stride, int pad_h, int pad_w,
                                 int dil, int Ho, int Wo, hipStream_t st);
PA_EXPORT int pa_conv2d_nhwc_fwd_stats(const void* x, const void* w, const void* bias, void* out, const void* zero,
                                       int N, int H, int W, int C, int Cout, int KH, int KW, int stride, int pad_h,
                                       int pad_w, int dil, int Ho, int Wo, float* stats, hipStream_t st);
PA_EXPORT int pa_conv2d_nhwc_fwd_bnbwd(const void* x, const void* w, void* out, const void* zero, int N, int H, int W,
                                       int C, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int dil,
                                       int Ho, int Wo, const void* bn_x, const float* bn_ss, const float* bn_mean,
                                       float* stats, hipStream_t st);
PA_EXPORT int pa_conv2d_nhwc_wgrad(const void* x, const void* dy, float* ws, const void* zero, int N, int H, int W,
                                   int C, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int dil, int Ho,
                                   int Wo, int splits, int bn, hipStream_t st);
PA_EXPORT int pa_gemm_small_m(const void* a, int64_t lda, const void* b, int64_t ldb, void* c, int64_t ldc,
                              const void* bias, float* ws, int M, int N, int K, int splits, int stages,
                              hipStream_t st);
PA_EXPORT int pa_slab_reduce_bf16(const float* ws, void* c, int64_t ldc, int64_t M, int64_t N, int splits,
                                  hipStream_t st);

// gemm_fp8.hip
PA_EXPORT int64_t pa_gemm_fp8_ws_bytes(int64_t M, int64_t N, int64_t K);
PA_EXPORT int pa_gemm_fp8(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                          int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha, int act,
                          int out_f16, hipStream_t st);
PA_EXPORT int pa_gemm_fp8_ws(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                             int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha, int act,
                             int out_f16, void* ws, hipStream_t st);
PA_EXPORT int pa_gemm_fp8_dscale(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N,
                                 int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha,
                                 int act, int out_f16, void* ws, const float* a_scale_inv, const float* b_scale_inv,
                                 hipStream_t st);
PA_EXPORT int pa_gemm_fp8_set_kernel(int k);

// gemm_skinny.hip
PA_EXPORT int pa_gemm_skinny_ok(int64_t N, int64_t K);
PA_EXPORT int pa_gemm_skinny(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                             int64_t lda, int64_t ldb, int64_t ldc, int b_kmajor, int flags, void* stream);
PA_EXPORT int64_t pa_gemm_skinny_stats_chunks(int64_t M, int64_t N, int64_t K);
PA_EXPORT int pa_gemm_skinny_stats(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N,
                                   int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int b_kmajor, float* stats,
                                   void* stream);
PA_EXPORT int pa_conv_skinny_ok(int64_t C, int64_t Cout, int64_t KH, int64_t KW);
PA_EXPORT int pa_conv_skinny(const void* x, const void* w, const void* bias, void* y, const void* zero_page,
                             int64_t N, int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t KH, int64_t KW,
                             int64_t stride, int64_t pad, int64_t Ho, int64_t Wo, void* stream);
PA_EXPORT int64_t pa_conv_skinny_stats_chunks(int64_t N, int64_t H, int64_t W);
PA_EXPORT int pa_conv_skinny_stats(const void* x, const void* w, const void* bias, void* y, const void* zero_page,
                                   int64_t N, int64_t H, int64_t W, float* stats, void* stream);
PA_EXPORT int pa_conv_skinny_wgrad(const void* x, const void* dy, const void* zero_page, float* ws, int64_t N,
                                   int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t splits, void* stream);

// grouped_gemm.hip
PA_EXPORT int pa_grouped_gemm(int mode, const void* a, const void* b, void* c, const void* bias, const int* offs,
                              const void* zero, int E, int64_t rows, int M, int N, int K, int64_t lda, int64_t ldb,
                              int64_t ldc, int flags, hipStream_t st);
PA_EXPORT int pa_moe_route(const int* eid, int n, int E, int* counts, int* offs, int* perm, hipStream_t st);

// lamb.hip
PA_EXPORT int pa_lamb_multi(const int64_t* table, const int64_t* items, int64_t n_items, const int64_t* offsets,
                            int64_t n_tensors, float* partial, float* trust, const float* inv_scale, float lr,
                            float b1, float b2, float eps, float bc1, float bc2, int always_adapt, hipStream_t st);

// linear_epi.hip
PA_EXPORT int pa_colsum(const void* x, void* out, float* ws, int64_t rows, int64_t cols, int dtype_acc,
                        hipStream_t st);
PA_EXPORT int pa_bias_gelu_bwd(const void* h, const void* b, const void* dy, void* dh, void* db, float* ws,
                               int64_t rows, int64_t cols, int dtype_acc, hipStream_t st);
PA_EXPORT int pa_dropout_add_fwd(const void* x, const void* res, void* out, int64_t n, float p, uint64_t seed,
                                 int dtype, hipStream_t st);
PA_EXPORT int pa_dropout_bwd(const void* dy, void* dx, int64_t n, float p, uint64_t seed, int dtype, hipStream_t st);
PA_EXPORT int pa_dropout_bwd_colsum(const void* dy, void* dx, float* ws, int64_t rows, int64_t cols, float p,
                                    uint64_t seed, int dtype, hipStream_t st);
PA_EXPORT int64_t pa_colsum_nparts(int64_t rows);
PA_EXPORT int pa_fold_partials(const float* ws, void* out, int64_t cols, int64_t nparts, int dtype_acc,
                               hipStream_t st);

// norm.hip
PA_EXPORT int pa_rms_norm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t cols,
                              float eps, int dtype, hipStream_t st);
PA_EXPORT int pa_rms_norm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx,
                              float* dw_part, int64_t rows, int64_t cols, int dtype_np, hipStream_t st);
PA_EXPORT int pa_rms_norm_bwd_res(const void* dy, const void* x, const void* w, const float* rstd, void* dx,
                                  float* dw_part, void* res, int64_t rows, int64_t cols, int dtype_np,
                                  hipStream_t st);
PA_EXPORT int pa_layer_norm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd,
                                int64_t rows, int64_t cols, float eps, int dtype, hipStream_t st);
PA_EXPORT int pa_layer_norm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                                void* dx, float* dw_part, float* db_part, void* res, int64_t rows, int64_t cols,
                                int dtype_np, hipStream_t st);
PA_EXPORT int pa_reduce_parts(const float* pa, const float* pb, void* oa, void* ob, int nparts, int64_t cols, int dta,
                              int dtb, hipStream_t st);
PA_EXPORT int pa_version();

// pool.hip
PA_EXPORT int pa_maxpool_nhwc_fwd(const void* x, void* y, void* arg, int N, int H, int W, int C, int Ho, int Wo,
                                  int K, int s, int p, int dtype, hipStream_t st);
PA_EXPORT int pa_maxpool_nhwc_bwd(const void* dy, const void* arg, void* dx, int N, int H, int W, int C, int Ho,
                                  int Wo, int K, int s, int p, int dtype, hipStream_t st);

// quant_fp8.hip
PA_EXPORT int64_t pa_fp8_nparts();
PA_EXPORT int pa_fp8_amax(const void* x, int64_t n, int dtype, float* parts, hipStream_t st);
PA_EXPORT int pa_fp8_scale_update(const float* parts, int n_parts, float* history, int hist_len, float* scale,
                                  float* scale_inv, float fmax, int margin, int mode, hipStream_t st);
PA_EXPORT int pa_fp8_quant(const void* x, int64_t R, int64_t C, int in_dtype, int fmt, const float* scale, void* q,
                           void* qT, float* parts, hipStream_t st);

// softmax.hip
PA_EXPORT int pa_softmax_fwd(const void* x, void* y, int64_t rows, int64_t cols, int dtype, hipStream_t st);
PA_EXPORT int pa_softmax_bwd(const void* y, const void* dy, void* dx, int64_t rows, int64_t cols, int dtype,
                             hipStream_t st);
PA_EXPORT int pa_softmax_ce_fwd(const void* logits, const int64_t* labels, float* loss, float* lse, int64_t rows,
                                int64_t cols, int64_t ignore_index, int dtype, hipStream_t st);
PA_EXPORT int pa_softmax_ce_bwd(const void* logits, const int64_t* labels, const float* lse, const float* dloss,
                                void* dlogits, int64_t rows, int64_t cols, int64_t ignore_index, int dtype,
                                hipStream_t st);
PA_EXPORT int pa_ce_slice_fwd(const void* logits, const int64_t* labels, float* lse, float* tgt, int64_t rows,
                              int64_t cols, int64_t v0, int dtype, hipStream_t st);
PA_EXPORT int pa_ce_slice_bwd(const void* logits, const int64_t* labels, const float* lse, const float* dloss,
                              void* dlogits, int64_t rows, int64_t cols, int64_t v0, int64_t ignore_index, int dtype,
                              hipStream_t st);

// wo_gemm.hip
PA_EXPORT int pa_wo_gemm_splits(int64_t M, int64_t N, int64_t K, int llm);
PA_EXPORT int pa_wo_gemm(const void* x, const void* xo, const float* sx, const void* w, const float* scale,
                         const void* bias, void* y, float* ws, int M, int N, int K, int ldx, int ldy, int bits,
                         int group, int splits, hipStream_t st);
PA_EXPORT int pa_wo_dequant(const void* w, const float* scale, void* out, int N, int K, int bits, int group,
                            hipStream_t st);
