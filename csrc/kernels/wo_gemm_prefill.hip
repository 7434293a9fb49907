// Weight-only int8 / int4 linear for prefill shapes: y[M, N] bf16 = x[M, K] bf16 . dequant(Wq)^T (+ bias) as one GEMM
// that reads the codes themselves. No bf16 image of the weight exists in memory; wo_gemm.hip covers M <= 64.
// Layouts are weight_quantize's, as in wo_gemm.hip: int8 [N, K]; int4 pair-rows [N / 2, K] (channels 2j / 2j + 1 in
// the low / high nibble, stored + 8, all 16 codes and all 256 int8 codes decode); scales fp32 [N] or [K / G, N] with
// G = 64 or 128.
//
// One kernel template, wo_prefill_k<BITS, G, TM>: a TM x 256 tile (TM = 256, or 128 for short inputs), 8 waves as
// 2 (M) x 4 (N), K tiles of 64 in two LDS stages of A TM x 128 B + B 32 KiB of bf16 (128 KiB at TM = 256), the
// swizzled K-major image frag<R, true> of mfma_tile.h reads; v_mfma_f32_16x16x32_bf16 with operands swapped as in
// moe_grouped_wo_k, so a lane ends with 4 consecutive channels of one row.
//   * A (bf16) goes global -> LDS by LDS-DMA, the k_swz swizzle in the per-lane source address. Rows past M re-read
//     the last row and are never stored.
//   * B (codes): a lane loads 16 bytes of codes along K two K tiles ahead of the MFMAs, converts them once (once per
//     weight element per workgroup: the 256-row tile halves the conversions per output row of the 128-row one) and
//     writes two 16-byte chunks of the image; an int4 pair-row load fills two image rows (wo_cvt.h).
//   * per-channel scales: the image holds the exact integers and the scale multiplies the finished fp32 sum.
//     Group scales: a K tile never straddles a group, so the lane loads the fp32 scale of its image row and K tile
//     with the codes and writes bf16(code * s), rounded to nearest even: the element pa_wo_dequant writes, so the
//     group modes keep the numerics of the bf16 GEMM on the dequantised image and need no second accumulator set.
//   * the last M tile and the last N band are ragged (N % 64 == 0: whole waves): channels past N are clamped reads,
//     and a wave whose 16-row fragments all lie past M, or whose channels lie past N, skips its LDS reads and MFMAs
//     (wave-uniform; it still stages and meets the barriers). A partly filled wave tile computes every fragment on
//     the clamped rows and stores only the rows below M.
//   * K split (gridDim.y): 256 <= M <= ~1024 against N = 4096 is 16 .. 64 tiles for 256 CUs, so the launcher picks
//     the tile height and a split of the K tiles that fill the chip (pa_wo_gemm_prefill_plan). A split writes its
//     unscaled fp32 sums to slab [split][M][N], every element exactly once; wo_prefill_finalize_k sums the slabs in
//     ascending order, applies the per-channel scale and the bias and writes bf16. No memset and no atomics: the same
//     bits every run. Without a split the epilogue applies scale and bias and stores bf16.
//
// Limits (the launcher returns non-zero otherwise): M >= 1, K % 64 == 0, N % 64 == 0, ldx % 8 == ldy % 8 == 0 with
// ldx >= K and ldy >= N (16-byte aligned rows), bits 8 / 4, group -1 / 64 / 128, tile_m 128 / 256 (0: the plan's),
// splits a divisor of K / 64 (0: the plan's). Rows of x, y, the codes and the slabs are addressed in 64 bits.
#include "common.h"
#include "launch.h"
#include "mfma_tile.h"
#include "wo_cvt.h"

namespace pa {
namespace {

constexpr int kPfTN = 256;
constexpr int kPfMaxSplits = 8;  // the plan's cap: a split costs 8 M N bytes of slab traffic

struct WoPfArgs {
  const uint16_t* x;     // [M][ldx] bf16
  const uint8_t* w;      // int8 [N][K] or int4 pair-rows [N / 2][K]
  const float* scale;    // [N] or [K / G][N]
  const uint16_t* bias;  // [N] bf16 or null
  uint16_t* y;           // [M][ldy] bf16 (no split)
  float* ws;             // [splits][M][N] fp32 (split)
  int M, N, K, ldx, ldy, tiles_m, tiles_n, nks, splits;  // nks: K tiles of one split
};

template <int BITS, int G, int TM>
__global__ __launch_bounds__(512, 1) void wo_prefill_k(WoPfArgs p) {
  constexpr int TN = kPfTN;
  constexpr int MR = TM / 32, NR = 4;    // wave tile TM / 2 x 64
  constexpr int NL = BITS == 8 ? 2 : 1;  // 16-byte code loads a lane makes per K tile
  constexpr int NS = G == 0 ? 0 : NL;    // scale loads of the group modes: one per code load (int4: the pair's two)
  constexpr int NV = NL + NS;            // the waits below count on exactly NV loads a step
  constexpr int AIMG = TM * 128, STAGE = (TM + TN) * 128;  // bytes: a K tile is 64 bf16 = 128 B a row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  int tm, tn;
  tile_coords(xcd_remap((int)blockIdx.x, (int)gridDim.x), p.tiles_m, p.tiles_n, &tm, &tn);
  const int m0 = tm * TM, n0 = tn * TN;
  const int kt0 = (int)blockIdx.y * p.nks;  // first K tile of this split
  const int nk = p.nks;

  // A staging: wave-instruction q = 8 i + wave fills image rows 8 q + (lane >> 3), the lane's 16-byte chunk swizzled
  // by k_swz in its global source address
  const char* asrc[TM / 64];
#pragma unroll
  for (int i = 0; i < TM / 64; ++i) {
    const int row = (i * 8 + wave) * 8 + (lane >> 3);
    asrc[i] = reinterpret_cast<const char*>(p.x + (int64_t)min(m0 + row, p.M - 1) * p.ldx + (int64_t)kt0 * 64) +
              (((lane & 7) ^ k_swz(row)) << 4);
  }
  // B staging: load l of thread tid is the 16 codes k = 16 part .. 16 part + 15 of image row `row` (int4: of rows
  // row and row + 1, row even and clamped to an even channel), which are the image chunks 2 part and 2 part + 1.
  // ssrc: the group scale of load l's image row (int4: of rows row and row + 1, adjacent channels, as one 8-byte
  // load; the scale rows are only known to be 4-byte aligned).
  typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
  const uint8_t* bsrc[NL];
  const float* ssrc[NL];
  int bdst[NL][2];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int idx = l * 512 + tid, part = idx & 3;
    const int row = BITS == 8 ? idx >> 2 : 2 * (idx >> 2);
    const int chan = min(n0 + row, p.N - (BITS == 8 ? 1 : 2));
    bsrc[l] = p.w + (int64_t)(chan / (8 / BITS)) * p.K + (int64_t)kt0 * 64 + part * 16;
    bdst[l][0] = AIMG + row * 128 + (((2 * part) ^ k_swz(row)) << 4);
    bdst[l][1] = AIMG + row * 128 + (((2 * part + 1) ^ k_swz(row)) << 4);
    ssrc[l] = p.scale + chan;
  }
  uint4 raw[NL];
  float sc[2];
  auto load_b = [&](int t) {
#pragma unroll
    for (int l = 0; l < NL; ++l) raw[l] = *reinterpret_cast<const uint4*>(bsrc[l] + (int64_t)t * 64);
    if constexpr (G != 0) {
      const int64_t go = (int64_t)((kt0 + t) * 64 / G) * p.N;
      if constexpr (BITS == 8) {
        sc[0] = ssrc[0][go];
        sc[1] = ssrc[1][go];
      } else {
        const f32x2u v = *reinterpret_cast<const f32x2u*>(ssrc[0] + go);
        sc[0] = v[0];
        sc[1] = v[1];
      }
    }
  };
  auto stage_a = [&](int t, int buf) {
#pragma unroll
    for (int i = 0; i < TM / 64; ++i) glds16(asrc[i] + (int64_t)t * 128, smem + buf * STAGE + (i * 8 + wave) * 1024);
  };
  auto stage_b = [&](int buf) {  // raw -> bf16 -> image
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      uint4 c0, c1;
      if constexpr (G != 0) gwo_cvt_scaled<BITS, false>(raw[l], sc[BITS == 8 ? l : 0], c0, c1);
      else gwo_cvt<BITS, false>(raw[l], c0, c1);
      *reinterpret_cast<uint4*>(base + bdst[l][0]) = c0;
      *reinterpret_cast<uint4*>(base + bdst[l][1]) = c1;
      if constexpr (BITS == 4) {  // the odd channel of the pair: the next image row, the same swizzle (row is even)
        if constexpr (G != 0) gwo_cvt_scaled<4, true>(raw[l], sc[1], c0, c1);
        else gwo_cvt<4, true>(raw[l], c0, c1);
        *reinterpret_cast<uint4*>(base + bdst[l][0] + 128) = c0;
        *reinterpret_cast<uint4*>(base + bdst[l][1] + 128) = c1;
      }
    }
  };

  // 16-row fragments of this wave that hold rows below M; none when the wave's 64 channels lie past N
  const int wcol = n0 + wn * 64;
  const int nfr = wcol < p.N ? min(max((p.M - m0 - wm * (TM / 2) + 15) >> 4, 0), MR) : 0;

  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // The code (and scale) registers run two K tiles ahead of the MFMAs, the LDS image one. Every step issues its
  // LDS-DMA before its NV loads, so vmcnt(NV) retires the DMA and leaves the loads in flight across the barrier.
  // The loop exists twice: a wave with no fragment to compute only stages and meets the barriers, so the
  // accumulators of the others are updated in place on one straight path (a branch around the MFMAs inside one
  // loop made the compiler keep a second copy of them).
  auto kloop = [&](auto live) {
    load_b(0);
    stage_a(0, 0);
    stage_b(0);
    load_b(min(1, nk - 1));
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NV) : "memory");
    bar();
    for (int t = 0; t < nk; ++t) {
      const int cur = t & 1;
      if (t + 1 < nk) {
        stage_b(cur ^ 1);  // tile t + 1, loaded a step ago
        stage_a(t + 1, cur ^ 1);
        load_b(min(t + 2, nk - 1));
      }
      if constexpr (decltype(live)::value) {
        const char* aimg = smem + cur * STAGE;
        const char* bimg = aimg + AIMG;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8_t bf[NR];
#pragma unroll
          for (int j = 0; j < NR; ++j) bf[j] = frag<TN, true>(bimg, wn * 64 + j * 16, s, lane);
#pragma unroll
          for (int i = 0; i < MR; ++i) {
            const bf16x8_t af = frag<TM, true>(aimg, wm * (TM / 2) + i * 16, s, lane);
#pragma unroll
            for (int j = 0; j < NR; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af, acc[i][j], 0, 0, 0);
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NV) : "memory");
      bar();
    }
  };
  if (nfr == 0) {
    kloop(IntC<0>{});
    return;
  }
  kloop(IntC<1>{});

  // lane holds, of row mrow0 + 16 i, the channels wcol + 16 j + 4 g + 0..3
  const int g = lane >> 4;
  const int mrow0 = m0 + wm * (TM / 2) + (lane & 15);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int c = wcol + 16 * j + 4 * g;
    if (p.splits > 1) {
      float* slab = p.ws + (int64_t)blockIdx.y * p.M * p.N;
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int m = mrow0 + i * 16;
        if (i >= nfr || m >= p.M) continue;
        *reinterpret_cast<float4*>(slab + (int64_t)m * p.N + c) =
            make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      }
    } else {
      float s[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (G == 0) {
        const float4 v = *reinterpret_cast<const float4*>(p.scale + c);
        s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
      }
      if (p.bias) load4_16(p.bias + c, b);
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int m = mrow0 + i * 16;
        if (i >= nfr || m >= p.M) continue;
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = acc[i][j][q] * s[q] + b[q];
        *reinterpret_cast<uint2*>(p.y + (int64_t)m * p.ldy + c) = make_uint2(pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]));
      }
    }
  }
}

// y = (slab 0 + slab 1 + ...) * scale (per-channel modes; null for the group modes) + bias, 4 channels a thread
__global__ __launch_bounds__(256) void wo_prefill_finalize_k(const float* ws, const float* scale, const uint16_t* bias,
                                                             uint16_t* y, int M, int N, int ldy, int splits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, nq = N / 4;
  if (i >= (int64_t)M * nq) return;
  const int64_t m = i / nq;
  const int c = (int)(i % nq) * 4;
  const float* src = ws + m * N + c;
  float4 v = *reinterpret_cast<const float4*>(src);
  for (int z = 1; z < splits; ++z) {
    const float4 u = *reinterpret_cast<const float4*>(src + (int64_t)z * M * N);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  if (scale) {
    const float4 s = *reinterpret_cast<const float4*>(scale + c);
    v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w;
  }
  if (bias) {
    float b[4];
    load4_16(bias + c, b);
    v.x += b[0]; v.y += b[1]; v.z += b[2]; v.w += b[3];
  }
  *reinterpret_cast<uint2*>(y + m * ldy + c) = make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w));
}

template <int BITS, int G>
int launch_prefill(const WoPfArgs& p, int tile_m, hipStream_t st) {
  const dim3 g((unsigned)(p.tiles_m * p.tiles_n), (unsigned)p.splits), b(512);
  return tile_m == 256 ? launch_lds<wo_prefill_k<BITS, G, 256>>(g, b, 2 * (256 + kPfTN) * 128, st, p)
                       : launch_lds<wo_prefill_k<BITS, G, 128>>(g, b, 2 * (128 + kPfTN) * 128, st, p);
}

bool prefill_shape_ok(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0 && M < (1ll << 31) && N < (1ll << 31) &&
         K < (1ll << 31) && cdiv(M, 128) * cdiv(N, kPfTN) < (1ll << 31);
}

}  // namespace
}  // namespace pa

using namespace pa;

// The launcher's choice of tile height and K split for a shape: the 256-row tile when its tiles alone fill the CUs,
// else the 128-row tile (twice the workgroups, so half the split: a split costs 8 M N bytes of slab traffic, more
// than the conversions the taller tile saves); then the smallest divisor of K / 64 (at most 8) with which
// tiles x splits reaches the CU count, or the largest such divisor. The workspace a caller passes is
// splits * M * N fp32 when splits > 1. Returns 1 for a shape pa_wo_gemm_prefill refuses.
PA_EXPORT int pa_wo_gemm_prefill_plan(int64_t M, int64_t N, int64_t K, int* tile_m, int* splits) {
  if (!prefill_shape_ok(M, N, K)) return 1;
  const int64_t cus = device_cus(), bands = cdiv(N, kPfTN);
  const int64_t t256 = cdiv(M, 256) * bands, t128 = cdiv(M, 128) * bands;
  const int tm = t256 >= cus ? 256 : 128;
  const int64_t tiles = tm == 256 ? t256 : t128, nk = K / 64;
  int s = 1;
  for (int d = 1; d <= kPfMaxSplits && d <= nk; ++d) {
    if (nk % d) continue;
    s = d;
    if (tiles * d >= cus) break;
  }
  *tile_m = tm;
  *splits = s;
  return 0;
}

// y [M, ldy] bf16 = x [M, ldx] bf16 . dequant(w)^T (+ bias [N] bf16 or null). bits: 8 / 4; group: -1 (scale [N]),
// 64 or 128 (scale [K / G, N]); tile_m: 128 / 256, splits: a divisor of K / 64 (0 for either: the plan's choice);
// ws: splits * M * N fp32 when splits > 1 (need not be cleared). Returns non-zero for what it refuses.
PA_EXPORT int pa_wo_gemm_prefill(const void* x, const void* w, const float* scale, const void* bias, void* y,
                                 float* ws, int M, int N, int K, int ldx, int ldy, int bits, int group, int tile_m,
                                 int splits, hipStream_t st) {
  if (!prefill_shape_ok(M, N, K) || ldx % 8 != 0 || ldy % 8 != 0 || ldx < K || ldy < N) return 1;
  if (bits != 8 && bits != 4) return 2;
  if (group != -1 && group != 64 && group != 128) return 3;
  int ptm = 0, ps = 0;
  if (pa_wo_gemm_prefill_plan(M, N, K, &ptm, &ps)) return 1;
  if (tile_m == 0) tile_m = ptm;
  if (splits == 0) splits = ps;
  if (tile_m != 128 && tile_m != 256) return 4;
  if (splits < 1 || splits > 65535 || (K / 64) % splits != 0) return 5;
  if (splits > 1 && ws == nullptr) return 6;
  WoPfArgs p{};
  p.x = (const uint16_t*)x; p.w = (const uint8_t*)w; p.scale = scale; p.bias = (const uint16_t*)bias;
  p.y = (uint16_t*)y; p.ws = ws;
  p.M = M; p.N = N; p.K = K; p.ldx = ldx; p.ldy = ldy;
  p.tiles_m = (M + tile_m - 1) / tile_m; p.tiles_n = (N + kPfTN - 1) / kPfTN;
  p.nks = K / 64 / splits; p.splits = splits;
  int rc;
  if (bits == 8) {
    rc = group == -1 ? launch_prefill<8, 0>(p, tile_m, st)
                     : (group == 64 ? launch_prefill<8, 64>(p, tile_m, st) : launch_prefill<8, 128>(p, tile_m, st));
  } else {
    rc = group == -1 ? launch_prefill<4, 0>(p, tile_m, st)
                     : (group == 64 ? launch_prefill<4, 64>(p, tile_m, st) : launch_prefill<4, 128>(p, tile_m, st));
  }
  if (rc) return rc;
  if (splits > 1) {
    const int64_t tot = (int64_t)M * (N / 4);
    hipLaunchKernelGGL(wo_prefill_finalize_k, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, ws,
                       group == -1 ? scale : nullptr, (const uint16_t*)bias, (uint16_t*)y, M, N, ldy, splits);
    return (int)hipGetLastError();
  }
  return 0;
}
