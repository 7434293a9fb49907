// MoE prefill over MXFP4 expert weights: the SwiGLU expert FFN of fused_moe(quant_method="mxfp4") for many tokens, as a
// grouped, row-gathering pair of block-scaled GEMMs with no host synchronisation:
//   pa_mx_quant (x -> mxfp8) -> up projection (+ bias + SwiGLU + mxfp8 quantisation of h) -> down projection -> combine.
// The operand formats are the decode path's (moe_decode.hip, the *_mx kernels; formats in mx.hip): x_q [T, d] e4m3fn +
// x_s [T, d / 32], w1_q [E, 2f, d / 2] + w1_s [E, 2f, d / 32] and w2_q [E, d, f / 2] + w2_s [E, d, f / 32] K-major per
// expert, biases bf16. Routing (val / idx, offs / perm of pa_moe_route, pos) is the caller's, on the device. The result
// is defined by ops.moe.moe_ffn_mx_reference.
//
// Both projections are mx.hip's gemm_mx_kernel with an mxfp8 A: a 128 x 256 tile, 8 waves as 2 (M) x 4 (N), two
// 64-KiB LDS stages of 256 k fed by LDS-DMA in the k_swz image (two fp8 A images + one fp4 B image a stage), the scale
// dwords straight from global memory, a half stage when K % 256 == 128, operands swapped so that a lane ends with 4
// channels of one row. That loop is copied, not re-scheduled. What is this file's own:
//   * the tile map of grouped_gemm.hip: M tiles are 128 sorted rows of one expert, the launch covers the upper bound
//     ceil(n / 128) + E of them (n = T * topk), a workgroup walks offs to its expert and row range and the tiles past
//     the last one exit at once; the host reads no count.
//   * the row maps. The LDS image and the fragment reads never change; which global row fills image row r does:
//       up, A:   the token perm[row] / topk of x_q (and of the row's scale dword in x_s): the gather is the per-lane
//                LDS-DMA source address, there is no gathered copy of x. Rows past the expert's end read its last row
//                and are never stored.
//       up, B:   128 value channels [c0, c0 + 128) and the 128 gate channels [f + c0, f + c0 + 128) of w1_q[e] as one
//                256-row image, ordered so that wave wn's 64 accumulator columns are the 32 value channels
//                c0 + 32 wn + [0, 32) (fragments 0, 1) and their 32 gate channels (fragments 2, 3), and inside them so
//                that the lane of k-group g = lane >> 4 holds the 8 consecutive channels 8 g + [0, 8): image row
//                64 wn + 16 j + w holds channel 32 wn + 8 (w >> 2) + 4 (j & 1) + (w & 3) of the half j >> 1.
//       down, A: the contiguous sorted rows of h_q / h_s, clamped at the expert's end; B: rows n0 + r of w2_q[e].
//   * the up epilogue, all on the accumulators: bias, silu(value) * gate, the amax of the row's 32-block (the 4 lanes
//     l, l + 16, l + 32, l + 48 hold a row's 32 channels: two cross-lane steps), the E8M0 byte and the e4m3 codes by
//     mx_block.h, the rule pa_mx_quant uses. A lane writes its 8 codes as one 8-byte store (a row's block is 32
//     contiguous bytes) and lane g == 0 the scale byte: h exists only as h_q [n, f] + h_s [n, f / 32].
//   * the down epilogue writes y [n, d] fp32, every sorted row exactly once (a row belongs to one expert and one M
//     tile): no memset, no atomic. moe_decode_combine_k (moe_combine.h) with one slab adds b2, weights by val and sums a
//     token's experts in ascending order, so the result has the same bits every run.
//
// Limits (the launchers return 1 otherwise): 1 <= T <= 65535 (the combine's gridDim.y), E <= 256, topk <= min(8, E),
// d % 128 == f % 128 == 0. Index arithmetic: rows of an expert's weights and of the scale arrays are addressed with
// 32-bit byte offsets from a 64-bit base, so d * f < 2^31 and n * max(d, f) < 2^36; rows of x_q, h_q and y are
// addressed in 64 bits.
#include "common.h"
#include "launch.h"
#include "mfma_tile.h"
#include "moe_combine.h"
#include "mx_block.h"

namespace pa {
namespace {

constexpr int kGmTM = 128, kGmTN = 256;
constexpr int kGmMaxT = 65535, kGmMaxE = 256, kGmMaxTopk = 8;

struct MoeGmxArgs {
  const uint8_t *aq, *as;  // up: x_q [T, d], x_s [T, d / 32]; down: h_q [n, f], h_s [n, f / 32]
  const uint8_t *bq, *bs;  // up: w1_q [E, 2f, d / 2], w1_s; down: w2_q [E, d, f / 2], w2_s
  const uint16_t* b1;      // [E, 2f] bf16 or null (up)
  const int *offs, *perm;  // [E + 1]; [n] sorted row -> entry (up)
  uint8_t *hq, *hs;        // up: [n, f] e4m3fn, [n, f / 32], sorted row order
  float* y;                // down: [n, d] fp32, sorted row order
  int T, E, topk, d, f, n, tiles_n;
};

// One 128 x 256 tile of one expert. UP: A = x_q gathered through perm, B = value + gate channels of w1_q[e], epilogue
// bias + SwiGLU + mxfp8 -> h_q / h_s. !UP: A = sorted rows of h_q, B = w2_q[e], epilogue fp32 y.
template <bool UP>
__device__ __forceinline__ void moe_grouped_mx_tile(const MoeGmxArgs& p) {
  constexpr int TM = kGmTM, TN = kGmTN;
  constexpr int MR = TM / 32, NR = 4;  // wave tile 64 x 64
  constexpr int kAImg = TM * 128, kABytes = 2 * kAImg, kStage = kABytes + TN * 128;
  static_assert(kStage == 64 * 1024, "two stages of 64 KiB");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;

  // tile map: the expert and the sorted rows [m0, mend) of M tile mt (offsets clamped into [0, n] and made monotonic,
  // so no plan can send a row outside the buffers)
  const int tn = (int)blockIdx.x % p.tiles_n, mt = (int)blockIdx.x / p.tiles_n;
  int e = -1, m0 = 0, mend = 0, cum = 0;
  for (int i = 0; i < p.E; ++i) {
    const int s = min(max(p.offs[i], 0), p.n), t = min(max(p.offs[i + 1], s), p.n);
    const int nt = (t - s + TM - 1) / TM;
    if (mt < cum + nt) {
      e = i; m0 = s + (mt - cum) * TM; mend = t;
      break;
    }
    cum += nt;
  }
  if (e < 0) return;  // past the last tile of the last expert (uniform over the workgroup)

  const int K = UP ? p.d : p.f, NB = UP ? 2 * p.f : p.d;  // reduction length, rows of one expert's B
  const int ldb = K / 2, lds = K / 32;
  const int n0 = tn * (UP ? TN / 2 : TN);
  const uint8_t* bq = p.bq + (int64_t)e * NB * ldb;
  const uint8_t* bs = p.bs + (int64_t)e * NB * lds;

  // the row maps: source row of A for tile row r, row of the expert's B for image row r
  auto a_row = [&](int r) {
    const int m = min(m0 + r, mend - 1);
    return UP ? min(max(p.perm[m] / p.topk, 0), p.T - 1) : m;
  };
  auto b_row = [&](int r) {
    if constexpr (UP) {
      const int j = (r >> 4) & 3, w = r & 15;
      return (j >> 1) * p.f + n0 + (r >> 6) * 32 + 8 * (w >> 2) + 4 * (j & 1) + (w & 3);
    } else {
      return min(n0 + r, p.d - 1);
    }
  };

  // staging (the image of mx.hip's stage_mx): wave-instruction q = 8 i + wave fills image rows 8 q + (lane >> 3), the
  // lane's 16-byte chunk swizzled by k_swz in its global source address
  const uint8_t* asrc[TM / 64];
  uint32_t bsrc[TN / 64];
#pragma unroll
  for (int i = 0; i < TM / 64; ++i) {
    const int row = (i * 8 + wave) * 8 + (lane >> 3);
    asrc[i] = p.aq + (int64_t)a_row(row) * K + (((lane & 7) ^ k_swz(row)) << 4);
  }
#pragma unroll
  for (int i = 0; i < TN / 64; ++i) bsrc[i] = (uint32_t)(b_row((i * 8 + wave) * 8 + (lane >> 3)) * ldb);

  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nks = K / 128;        // MFMA k-steps
  const int nst = (nks + 1) / 2;  // stages of 256 k
  auto stage_tile = [&](int t, int buf) {
    char* base = smem + buf * kStage;
#pragma unroll
    for (int i = 0; i < TM / 64; ++i) {
      glds16(asrc[i] + t * 256, base + (i * 8 + wave) * 1024);
      if (2 * t + 1 < nks) glds16(asrc[i] + t * 256 + 128, base + kAImg + (i * 8 + wave) * 1024);
    }
#pragma unroll
    for (int i = 0; i < TN / 64; ++i) {
      const int row = (i * 8 + wave) * 8 + (lane >> 3);
      // the k offset clamped inside the row: a half stage must not be read past the row's end
      const int kb = min(t * 128 + (((lane & 7) ^ k_swz(row)) << 4), ldb - 16);
      glds16(bq + bsrc[i] + kb, base + kABytes + (i * 8 + wave) * 1024);
    }
  };

  // scales, as in gemm_mx_kernel: the dword (4 k-blocks) of each fragment row for the two k-steps of the stage, the
  // lane's byte shifted down in front of the MFMA, refilled for the next stage after the row's last MFMA of this one
  const int sh = 8 * (lane >> 4);
  const int lo4 = frag_lo(lane, lane >> 4);
  uint32_t aoff[MR], boff[NR];
#pragma unroll
  for (int i = 0; i < MR; ++i) aoff[i] = (uint32_t)a_row(wm * (TM / 2) + i * 16 + (lane & 15)) * (uint32_t)lds;
#pragma unroll
  for (int j = 0; j < NR; ++j) boff[j] = (uint32_t)(b_row(wn * 64 + j * 16 + (lane & 15)) * lds);
  uint32_t sa[MR][2], sb[NR][2];
  auto hi_of = [&](int t) { return 2 * t + 1 < nks ? 4 : 0; };
  auto load_sa = [&](int i, int t) {
    const uint8_t* s = p.as + 8 * t;
    sa[i][0] = *reinterpret_cast<const uint32_t*>(s + aoff[i]);
    sa[i][1] = *reinterpret_cast<const uint32_t*>(s + hi_of(t) + aoff[i]);
  };
  auto load_sb = [&](int j, int t) {
    const uint8_t* s = bs + 8 * t;
    sb[j][0] = *reinterpret_cast<const uint32_t*>(s + boff[j]);
    sb[j][1] = *reinterpret_cast<const uint32_t*>(s + hi_of(t) + boff[j]);
  };

#pragma unroll
  for (int i = 0; i < MR; ++i) load_sa(i, 0);
#pragma unroll
  for (int j = 0; j < NR; ++j) load_sb(j, 0);
  stage_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nst; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < nst;    // then this stage has both k-steps
    const int tr = more ? t + 1 : t;  // the stage the scale registers are refilled for (the last one: itself, unused)
    if (more) stage_tile(t + 1, cur ^ 1);
    const char* aimg = smem + cur * kStage;
    const char* bimg = aimg + kABytes;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * t + s < nks) {
        i32x8 bf[NR];
        int bsc[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          bf[j] = frag4(bimg + (wn * 64 + j * 16) * 128, lo4, s);
          bsc[j] = (int)((sb[j][s] >> sh) & 0xffu);
        }
#pragma unroll
        for (int i = 0; i < MR; ++i) {
          const i32x8 af = frag8(aimg + s * kAImg + (wm * (TM / 2) + i * 16) * 128, lo4);
          const int asc = (int)((sa[i][s] >> sh) & 0xffu);
#pragma unroll
          for (int j = 0; j < NR; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af, acc[i][j], kFmtFp4, kFmtFp8, 0,
                                                                         bsc[j], 0, asc);
          if (s == 1) load_sa(i, tr);
        }
        if (s == 1) {
#pragma unroll
          for (int j = 0; j < NR; ++j) load_sb(j, tr);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // lane holds, of sorted row mrow0 + 16 i, the accumulator columns 64 wn + 16 j + 4 g + 0..3
  const int g = lane >> 4;
  const int mrow0 = m0 + wm * (TM / 2) + (lane & 15);
  if constexpr (UP) {
    // columns 16 j + 4 g + q of fragments j = 0, 1 are value channels cb + 8 g + 4 j + q, of j = 2, 3 their gates
    const int cb = n0 + wn * 32;  // the wave's 32-block of h
    float ba[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p.b1) {
      const uint16_t* b = p.b1 + (int64_t)e * 2 * p.f + cb + 8 * g;
      load4_16(b, ba); load4_16(b + 4, ba + 4);
      load4_16(b + p.f, bg); load4_16(b + p.f + 4, bg + 4);
    }
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      float h[8];
      float amax = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        h[c] = silu(acc[i][c >> 2][c & 3] + ba[c]) * (acc[i][2 + (c >> 2)][c & 3] + bg[c]);
        amax = fmaxf(amax, fabsf(h[c]));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      const int eb = mx_block_exp<8>(amax);
      const float s = mx_block_mult(eb);
      const uint32_t w0 = mx_e4m3x2<true>(h[2], h[3], s, mx_e4m3x2<false>(h[0], h[1], s, 0));
      const uint32_t w1 = mx_e4m3x2<true>(h[6], h[7], s, mx_e4m3x2<false>(h[4], h[5], s, 0));
      const int m = mrow0 + i * 16;
      if (m < mend) {
        *reinterpret_cast<uint2*>(p.hq + (int64_t)m * p.f + cb + 8 * g) = make_uint2(w0, w1);
        if (g == 0) p.hs[(int64_t)m * (p.f / 32) + (cb >> 5)] = (uint8_t)eb;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int n = n0 + wn * 64 + j * 16 + 4 * g;
      if (n >= p.d) continue;  // d % 4 == 0
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int m = mrow0 + i * 16;
        if (m < mend)
          *reinterpret_cast<float4*>(p.y + (int64_t)m * p.d + n) =
              make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      }
    }
  }
}

__global__ __launch_bounds__(512, 1) void moe_grouped_up_mx_k(MoeGmxArgs p) { moe_grouped_mx_tile<true>(p); }
__global__ __launch_bounds__(512, 1) void moe_grouped_down_mx_k(MoeGmxArgs p) { moe_grouped_mx_tile<false>(p); }

bool moe_grouped_mx_shape_ok(int T, int E, int topk, int d, int f) {
  if (T < 1 || T > kGmMaxT || E < 1 || E > kGmMaxE || topk < 1 || topk > kGmMaxTopk || topk > E) return false;
  if (d < 128 || f < 128 || d % 128 != 0 || f % 128 != 0) return false;
  const int64_t n = (int64_t)T * topk;
  return (int64_t)d * f < (1ll << 31) && n * (d > f ? d : f) < (1ll << 36);
}

template <bool UP>
int launch_grouped_mx(MoeGmxArgs& p, hipStream_t st) {
  p.tiles_n = UP ? p.f / (kGmTN / 2) : (p.d + kGmTN - 1) / kGmTN;
  const int64_t grid = (int64_t)((p.n + kGmTM - 1) / kGmTM + p.E) * p.tiles_n;
  const dim3 g((unsigned)grid), b(512);
  constexpr int lds = 2 * 64 * 1024;
  return UP ? launch_lds<moe_grouped_up_mx_k>(g, b, lds, st, p) : launch_lds<moe_grouped_down_mx_k>(g, b, lds, st, p);
}

}  // namespace
}  // namespace pa

using namespace pa;

// Up projection of the MXFP4 expert FFN over expert-sorted rows: xq [T, d] e4m3fn + xs [T, d / 32] (pa_mx_quant of x,
// mxfp8), w1q [E, 2f, d / 2] + w1s [E, 2f, d / 32] (mxfp4, K-major per expert), b1 [E, 2f] bf16 or null, offs [E + 1] and
// perm [n] int32 as pa_moe_route leaves them (n = T * topk entries, all kept) -> hq [n, f] e4m3fn + hs [n, f / 32], the
// mxfp8 quantisation of silu(value) * gate in sorted row order (neither needs clearing). Returns 1 for a shape it does
// not take (the limits at the top of this file).
PA_EXPORT int pa_moe_grouped_up_mx(const void* xq, const void* xs, const void* w1q, const void* w1s, const void* b1,
                                   const int* offs, const int* perm, void* hq, void* hs, int T, int E, int topk, int d,
                                   int f, hipStream_t st) {
  if (!moe_grouped_mx_shape_ok(T, E, topk, d, f)) return 1;
  MoeGmxArgs p{};
  p.aq = (const uint8_t*)xq; p.as = (const uint8_t*)xs; p.bq = (const uint8_t*)w1q; p.bs = (const uint8_t*)w1s;
  p.b1 = (const uint16_t*)b1; p.offs = offs; p.perm = perm; p.hq = (uint8_t*)hq; p.hs = (uint8_t*)hs;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk;
  return launch_grouped_mx<true>(p, st);
}

// Down projection and combine: hq / hs as pa_moe_grouped_up_mx leaves them, w2q [E, d, f / 2] + w2s [E, d, f / 32],
// b2 [E, d] bf16 or null, val [T, topk] fp32, idx [T, topk] and pos [n] (entry -> sorted row) int32, y = n * d fp32 of
// workspace (need not be cleared) -> out [T, d] bf16. Returns 1 for a shape it does not take.
PA_EXPORT int pa_moe_grouped_down_mx(const void* hq, const void* hs, const void* w2q, const void* w2s, const void* b2,
                                     const float* val, const int* idx, const int* offs, const int* pos, float* y,
                                     void* out, int T, int E, int topk, int d, int f, hipStream_t st) {
  if (!moe_grouped_mx_shape_ok(T, E, topk, d, f)) return 1;
  MoeGmxArgs p{};
  p.aq = (const uint8_t*)hq; p.as = (const uint8_t*)hs; p.bq = (const uint8_t*)w2q; p.bs = (const uint8_t*)w2s;
  p.offs = offs; p.y = y;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk;
  const int rc = launch_grouped_mx<false>(p, st);
  if (rc) return rc;
  MoeDecArgs c{};
  c.b2 = (const uint16_t*)b2; c.val = val; c.idx = idx; c.pos = pos; c.ws = y; c.out = (uint16_t*)out;
  c.T = T; c.E = E; c.topk = topk; c.d = d; c.f = f; c.n = p.n; c.splits = 1;
  hipLaunchKernelGGL(moe_decode_combine_k, dim3((d / 4 + 255) / 256, T), dim3(256), 0, st, c);
  return (int)hipGetLastError();
}
