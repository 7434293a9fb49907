// OCP fp8 GEMM on the gfx950 block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) with a fused
// epilogue: C[M,N] = act(alpha * A[M,K] . B[N,K]^T + bias[N]), C in fp16 or bf16.
// Reference behaviour: python/paddle/tensor/linalg.py fp8_fp8_half_gemm_fused and
// paddle/phi/kernels/fusion/fp8_gemm/ (cutlass fp8 GEMM with bias + identity / relu / gelu epilogue).
//
// A and B are both K-major (x [M][K] and the weight stored [N][K], transpose_y=True in the reference);
// the Python wrapper makes other layouts K-major first. Either operand may be e4m3 or e5m2
// (cbsz / blgp format codes 0 / 1). The per-tensor scale of the reference is `alpha`, applied in the
// epilogue, times the operands' scale inverses read from device memory when given (pa_gemm_fp8_dscale: the
// scales quant_fp8.hip computes on the device never cross to the host); the MFMA's per-32-element E8M0 block scales are all 1.0 (exponent 127), so the
// instruction runs the MX-fp8 rate (2x bf16 per clock) on plain per-tensor-scaled data.
//
// Structure: the bf16 generic kernel's (gemm.hip gemm_bf16_kernel) at the same bytes: 256 x 256 tiles,
// 128 k (= 128 bytes) per stage, 8 waves as 2 (M) x 4 (N) with a 128 x 64 wave tile, two LDS stages of
// 64 KiB fed by LDS-DMA, 16-B chunk XOR swizzle on 128-B rows (stage<R, true> of mfma_tile.h on bytes: the
// bf16 K-major image byte for byte). Fragments: lane l holds row (l & 15) and the 32 k-bytes [32 (l >> 4), 32 (l >> 4) + 32) for A and for B alike, so any k permutation
// the instruction applies inside its 128-k block is the same on both operands (and with unit block scales
// no scale placement matters). Operands are swapped (D = B-frag x A-frag) so a lane ends with 4
// consecutive columns of one output row.
#include "common.h"
#include "gemm_plan.h"
#include "launch.h"
#include "mfma_tile.h"
#include "pingpong256.h"

using namespace pa;

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int kTile = 256;
constexpr int kKB = 128;  // bytes (= fp8 elements) of k per stage
constexpr int kOpBytes = kTile * kKB;
constexpr int kStage = 2 * kOpBytes;

struct Fp8Args {
  const uint8_t* a;
  const uint8_t* b;
  void* c;
  const uint16_t* bias;
  int64_t lda, ldb, ldc;
  int M, N, K;
  int tiles_m, tiles_n;
  float alpha;
  int act;  // 0 identity, 1 gelu (erf), 2 relu
  // per-tensor dequantisation scales in device memory (one fp32 each, or null = 1): the epilogues multiply alpha by
  // them, so a scale computed on the device never crosses to the host
  const float* a_scale_inv;
  const float* b_scale_inv;
  // balanced tail (ping-pong kernel, as gemm.hip's): tiles [full_tiles, tiles) are cut along K into tail_split
  // slices that write fp32 256 x 256 partials to tail_ws; gemm_fp8_tail_reduce_k sums them and applies the epilogue
  int full_tiles, tail_split;
  float* tail_ws;
};

// fragment of a stage<R, true> image [R][128 B]: the lane's two chunks of its row, k_swz undone
__device__ __forceinline__ i32x8 frag(const char* img, int rbase, int lane) {
  const int row = rbase + (lane & 15);
  const int c0 = 2 * (lane >> 4), sw = k_swz(row);
  // chunks c0, c0 + 1 (c0 even) sit at (c0 ^ sw) and (c0 ^ sw) ^ 1: the second address is the first XOR 16
  const int off = row * 128 + ((c0 ^ sw) << 4);
  const uint4 lo = *reinterpret_cast<const uint4*>(img + off);
  const uint4 hi = *reinterpret_cast<const uint4*>(img + (off ^ 16));
  i32x8 f;
  f[0] = (int)lo.x; f[1] = (int)lo.y; f[2] = (int)lo.z; f[3] = (int)lo.w;
  f[4] = (int)hi.x; f[5] = (int)hi.y; f[6] = (int)hi.z; f[7] = (int)hi.w;
  return f;
}

// alpha times the device-side scales, formed once per workgroup before its epilogue loop (null pointers: alpha itself)
__device__ __forceinline__ float alpha_eff(const Fp8Args& p) {
  return p.alpha * (p.a_scale_inv ? *p.a_scale_inv : 1.f) * (p.b_scale_inv ? *p.b_scale_inv : 1.f);
}

__device__ __forceinline__ float act_f(float v, int act) {
  if (act == 1) return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  if (act == 2) return v > 0.f ? v : 0.f;
  return v;
}

template <int FA, int FB, bool OUT_F16>
__global__ __launch_bounds__(512, 1) void gemm_fp8_kernel(Fp8Args p) {
  constexpr int MR = 8, NR = 4;  // wave tile 128 x 64
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;

  const int nwg = p.tiles_m * p.tiles_n;
  const int pid = xcd_remap((int)blockIdx.x, nwg);
  int tm, tn;
  tile_coords(pid, p.tiles_m, p.tiles_n, &tm, &tn);
  const int m0 = tm * kTile, n0 = tn * kTile;

  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto stage_tile = [&](int t, int buf) {
    char* base = smem + buf * kStage;
    stage<kTile, true>(p.a, p.lda, m0, p.M, t * kKB, base, wave, lane);
    stage<kTile, true>(p.b, p.ldb, n0, p.N, t * kKB, base + kOpBytes, wave, lane);
  };

  const int nk = p.K / kKB;
  stage_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk) stage_tile(t + 1, cur ^ 1);
    const char* aimg = smem + cur * kStage;
    const char* bimg = aimg + kOpBytes;
    i32x8 bf[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) bf[j] = frag(bimg, wn * 64 + j * 16, lane);
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const i32x8 af = frag(aimg, wm * 128 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < NR; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af, acc[i][j], FB, FA, 0, 127, 0, 127);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // lane holds C[m = mrow0 + i*16][n = ncol0 + j*16 + 0..3]
  const int mrow0 = m0 + wm * 128 + (lane & 15);
  const int ncol0 = n0 + wn * 64 + 4 * (lane >> 4);
  const float alpha = alpha_eff(p);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int n = ncol0 + j * 16;
    if (n >= p.N) continue;  // N % 4 == 0 (launcher)
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) load4_16<OUT_F16>(p.bias + n, bv);
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const int m = mrow0 + i * 16;
      if (m >= p.M) continue;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_f(acc[i][j][e] * alpha + bv[e], p.act);
      uint2* cp = reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.c) + (int64_t)m * p.ldc + n);
      *cp = OUT_F16 ? make_uint2(pack_f16(v[0], v[1]), pack_f16(v[2], v[3]))
                    : make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Ping-pong fp8 kernel: the 256x256 8-phase schedule of pingpong256.h (PPLoop, the one gemm.hip's
// gemm256_kernel runs) at the fp8 byte geometry. A K-tile of 128 fp8 is 128 bytes per row — the bf16 kernel's
// 64-element tile byte for byte — so the half-tiles, the issue distance, the counted vmcnt waits, the barrier
// stagger and the LDS swizzle are that header's; per phase a wave runs 8 v_mfma_f32_16x16x128_f8f6f4 (= the 16
// bf16 16x16x32 MFMAs' cycles at twice the FLOPs). This file supplies the fp8 policy: lane l holds row (l & 15) and
// k-bytes [32 (l >> 4), +32) of the 128-byte row (chunks 2g, 2g + 1). The tail-slice decode, the partial store and
// the one-pass 16-bit epilogue (alpha, bias, activation in registers, the tile staged through LDS, 16-byte row
// stores; N % 8 == 0) are the shared ones too.

// C += B-frag x A-frag on the unscaled v_mfma_f32_16x16x128_f8f6f4 (formats in cbsz / blgp); PA_FP8_SCALED_MFMA
// selects the block-scaled form with unit E8M0 scales instead (the builtin: an extra scale operand pair).
template <int FA, int FB>
__device__ __forceinline__ f32x4 mfma8(const i32x8& b, const i32x8& a, f32x4 c) {
#ifdef PA_FP8_SCALED_MFMA
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, FB, FA, 0, 127, 0, 127);
#else
  if constexpr (FB == 0 && FA == 0) {
    asm("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0" : "+v"(c) : "v"(b), "v"(a));
  } else if constexpr (FB == 1 && FA == 0) {
    asm("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0 cbsz:1" : "+v"(c) : "v"(b), "v"(a));
  } else if constexpr (FB == 0 && FA == 1) {
    asm("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0 blgp:1" : "+v"(c) : "v"(b), "v"(a));
  } else {
    asm("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %0 cbsz:1 blgp:1" : "+v"(c) : "v"(b), "v"(a));
  }
  return c;
#endif
}

// balanced-tail reduction: tail tile b = tile full_tiles + b; a thread sums the slices' partials of 4 columns and
// applies the epilogue
template <bool OUT_F16>
__global__ __launch_bounds__(256) void gemm_fp8_tail_reduce_k(Fp8Args p) {
  const int b = blockIdx.x;
  int tm, tn;
  tile_coords(p.full_tiles + b, p.tiles_m, p.tiles_n, &tm, &tn);
  const int e = (blockIdx.y * 256 + threadIdx.x) * 4;
  const int r = e >> 8, c = e & 255;
  const int m = tm * 256 + r, n = tn * 256 + c;
  if (m >= p.M || n >= p.N) return;
  const float4 a = tail_sum4(p.tail_ws + (int64_t)b * p.tail_split * kPPTileElems + e, p.tail_split);
  float bq[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) load4_16<OUT_F16>(p.bias + n, bq);
  const float av[4] = {a.x, a.y, a.z, a.w};
  const float alpha = alpha_eff(p);
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = act_f(av[q] * alpha + bq[q], p.act);
  *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.c) + (int64_t)m * p.ldc + n) =
      OUT_F16 ? make_uint2(pack_f16(v[0], v[1]), pack_f16(v[2], v[3]))
              : make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
}

// The fp8 policy of PPLoop: one 16x16x128 MFMA per fragment pair and K-tile of 128, plain K-major bytes.
template <int FA, int FB>
struct PPFp8Ops {
  static constexpr int kSub = 1;
  using Frag = i32x8;
  const Fp8Args& p;
  int m0, n0, wave, lane;

  static __device__ __forceinline__ Frag read_a(const char* img, int rbase, int, int lane) {
    return frag(img, rbase, lane);
  }
  static __device__ __forceinline__ Frag read_b(const char* img, int rbase, int, int lane) {
    return frag(img, rbase, lane);
  }
  static __device__ __forceinline__ f32x4 mma(const Frag& b, const Frag& a, f32x4 c) { return mfma8<FA, FB>(b, a, c); }
  __device__ __forceinline__ void stage_half(int t, int h, char* dst) const {
    const int k0 = t * kKB;
    if (h == 0 || h == 2) stage<128, true>(p.a, p.lda, m0 + (h == 2 ? 128 : 0), p.M, k0, dst, wave, lane);
    else stage<128, true>(p.b, p.ldb, n0 + (h == 3 ? 128 : 0), p.N, k0, dst, wave, lane);
  }
};

template <int FA, int FB, bool OUT_F16>
__global__ __launch_bounds__(kPPThreads, 1) void gemm_fp8_pp_kernel(Fp8Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;

  const PPWork w = pp_work(p, (int)blockIdx.x);
  if (w.tail_out) {  // K slice of a tail tile
    p.a += (int64_t)w.ks * p.K;
    p.b += (int64_t)w.ks * p.K;
  }
  int tm, tn;
  tile_coords(w.pid, p.tiles_m, p.tiles_n, &tm, &tn);
  const int m0 = tm * kTile, n0 = tn * kTile;

  f32x4 acc[2][4][2][2];
  const PPFp8Ops<FA, FB> ops{p, m0, n0, wave, lane};
  const int nk = p.K / kKB;
  PPLoop<PPFp8Ops<FA, FB>> L{ops, smem, nk, wm, wn, lane, acc};
  L.start();
  int t = 0;  // the two K loops stay in the kernel: see PPLoop
#pragma unroll 1
  for (; t < L.nsteady(); ++t) L.ktile(t, IntC<1>{});
#pragma unroll 1
  for (; t < nk; ++t) L.ktile(t, IntC<0>{});
  L.finish();

  // The MFMAs are inline asm, so the compiler's hazard tracking does not see their results: wait out the
  // MFMA -> VALU read latency of the last accumulators explicitly.
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  if (w.tail_out) {
    pp_store_partial(w.tail_out, acc, wm, wn, lane);
    return;
  }

  // epilogue: alpha, bias, activation in registers; the 16-bit tile through LDS; row stores
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  pp_epilogue16(
      smem, acc, reinterpret_cast<uint16_t*>(p.c), p.ldc, p.M, p.N, m0, n0, alpha_eff(p), tid,
      [&](int n, float* bq) {
        if (p.bias && n < p.N) load4_16<OUT_F16>(p.bias + n, bq);
      },
      [&](float v) { return act_f(v, p.act); },
      [](float a, float b) { return OUT_F16 ? pack_f16(a, b) : pack_bf16(a, b); });
}

// ping-pong kernel with the balanced tail pl (the plan g.full_tiles / g.tail_split were filled from)
template <int FA, int FB, bool F16>
int launch_pp(const Fp8Args& g, const TailPlan& pl, hipStream_t st) {
  // two 64-KiB stages; the epilogue image [256][264] x 2 B (132 KiB) reuses them and is the larger
  const int rc = launch_lds<gemm_fp8_pp_kernel<FA, FB, F16>>(dim3(pl.grid), dim3(kPPThreads), kPPLds16, st, g);
  if (rc || !pl.split) return rc;
  hipLaunchKernelGGL((gemm_fp8_tail_reduce_k<F16>), dim3(pl.tiles - pl.full_tiles, 64), dim3(256), 0, st, g);
  return (int)hipGetLastError();
}

template <int FA, int FB, bool F16>
int launch(const Fp8Args& g, hipStream_t st) {
  return launch_lds<gemm_fp8_kernel<FA, FB, F16>>(dim3(g.tiles_m * g.tiles_n), dim3(512), 2 * kStage, st, g);
}

template <int FA, int FB>
int launch_out(const Fp8Args& g, int out_f16, bool pp, const TailPlan& pl, hipStream_t st) {
  if (pp) return out_f16 ? launch_pp<FA, FB, true>(g, pl, st) : launch_pp<FA, FB, false>(g, pl, st);
  return out_f16 ? launch<FA, FB, true>(g, st) : launch<FA, FB, false>(g, st);
}

// kernel choice: 0 auto (ping-pong when N % 8 == 0 and ldc % 8 == 0), 1 generic, 2 ping-pong (as auto)
int g_fp8_kernel = 0;

}  // namespace

// fmt_a / fmt_b: 0 = e4m3fn, 1 = e5m2. act: 0 identity, 1 gelu, 2 relu. bias: [N] in the output dtype or null.
// Returns 1 for an unsupported shape / stride (K % 128, N % 4, leading dims % 16 bytes).
// Workspace (bytes) the ping-pong fp8 GEMM's balanced tail needs (0: none).
PA_EXPORT int64_t pa_gemm_fp8_ws_bytes(int64_t M, int64_t N, int64_t K) {
  return tail_plan(M, N, K, kKB, device_cus()).ws_bytes;
}

static int fp8_impl(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                    int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha, int act, int out_f16,
                    void* ws, const float* a_scale_inv, const float* b_scale_inv, hipStream_t st);

PA_EXPORT int pa_gemm_fp8(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                          int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha, int act,
                          int out_f16, hipStream_t st) {
  return fp8_impl(a, b, c, bias, M, N, K, lda, ldb, ldc, fmt_a, fmt_b, alpha, act, out_f16, nullptr, nullptr, nullptr,
                  st);
}

// the same with the balanced-tail workspace (pa_gemm_fp8_ws_bytes(M, N, K) bytes; may be null when that is 0)
PA_EXPORT int pa_gemm_fp8_ws(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                             int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha, int act,
                             int out_f16, void* ws, hipStream_t st) {
  return fp8_impl(a, b, c, bias, M, N, K, lda, ldb, ldc, fmt_a, fmt_b, alpha, act, out_f16, ws, nullptr, nullptr,
                  st);
}

// pa_gemm_fp8_ws with the operands' dequantisation scales read from device memory: C = act(alpha * *a_scale_inv *
// *b_scale_inv * A . B^T + bias); either pointer may be null (= 1)
PA_EXPORT int pa_gemm_fp8_dscale(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N,
                                 int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha,
                                 int act, int out_f16, void* ws, const float* a_scale_inv, const float* b_scale_inv,
                                 hipStream_t st) {
  return fp8_impl(a, b, c, bias, M, N, K, lda, ldb, ldc, fmt_a, fmt_b, alpha, act, out_f16, ws, a_scale_inv,
                  b_scale_inv, st);
}

static int fp8_impl(const void* a, const void* b, void* c, const void* bias, int64_t M, int64_t N, int64_t K,
                    int64_t lda, int64_t ldb, int64_t ldc, int fmt_a, int fmt_b, float alpha, int act, int out_f16,
                    void* ws, const float* a_scale_inv, const float* b_scale_inv, hipStream_t st) {
  if (K % kKB != 0 || N % 4 != 0 || lda % 16 != 0 || ldb % 16 != 0 || ldc % 4 != 0) return 1;
  if (fmt_a < 0 || fmt_a > 1 || fmt_b < 0 || fmt_b > 1 || act < 0 || act > 2) return 1;
  if (M <= 0 || N <= 0) return 0;
  Fp8Args g{};
  g.a = (const uint8_t*)a; g.b = (const uint8_t*)b; g.c = c; g.bias = (const uint16_t*)bias;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.tiles_m = (int)((M + kTile - 1) / kTile);
  g.tiles_n = (int)((N + kTile - 1) / kTile);
  g.alpha = alpha; g.act = act;
  g.a_scale_inv = a_scale_inv; g.b_scale_inv = b_scale_inv;
  const bool pp = g_fp8_kernel != 1 && N % 8 == 0 && ldc % 8 == 0;
  TailPlan pl = tail_plan(M, N, K, kKB, device_cus());
  if (!pp || !ws) pl = without_tail(pl);
  g.full_tiles = pl.full_tiles;
  g.tail_split = pl.split;
  g.tail_ws = pl.split ? (float*)ws : nullptr;
  if (fmt_a == 0 && fmt_b == 0) return launch_out<0, 0>(g, out_f16, pp, pl, st);
  if (fmt_a == 0 && fmt_b == 1) return launch_out<0, 1>(g, out_f16, pp, pl, st);
  if (fmt_a == 1 && fmt_b == 0) return launch_out<1, 0>(g, out_f16, pp, pl, st);
  return launch_out<1, 1>(g, out_f16, pp, pl, st);
}

// 0 auto, 1 generic kernel only (A/B and tests)
PA_EXPORT int pa_gemm_fp8_set_kernel(int k) {
  g_fp8_kernel = k;
  return 0;
}
