// MoE prefill over weight-only int8 / int4 expert weights: the SwiGLU expert FFN of fused_moe(quant_method=
// "weight_only_int8" | "weight_only_int4") for many tokens, as a grouped, row-gathering pair of GEMMs that read the
// codes themselves: no bf16 image of the weights exists anywhere and the host reads nothing.
//   up projection (+ scale + bias + SwiGLU -> h bf16) -> down projection (+ scale -> y fp32) -> combine.
// The weight tensors are the decode path's (moe_decode_wo.hip): w1_q [E, 2f, d] int8 or [E, f, d] int4 pair-rows
// (channels 2j / 2j + 1 in the low / high nibble, stored + 8, all 16 codes decode), w1_s [E, 2f] fp32; w2_q [E, d, f]
// or [E, d / 2, f], w2_s [E, d] fp32; biases bf16. Routing (val / idx, offs / perm of pa_moe_route, pos) is the
// caller's, on the device. The result is defined by ops.moe.moe_ffn_wo_reference.
//
// One kernel template, moe_grouped_wo_k<BITS, UP>: a 128 x 256 tile, 8 waves as 2 (M) x 4 (N), K tiles of 64 in two
// 48-KiB LDS stages (A 16 KiB + B 32 KiB of bf16, the swizzled K-major image frag<R, true> of mfma_tile.h reads),
// v_mfma_f32_16x16x32_bf16 with operands swapped so that a lane ends with 4 consecutive channels of one row.
//   * the tile map of grouped_gemm.hip / moe_grouped_mx.hip: M tiles are 128 sorted rows of one expert, the launch
//     covers the upper bound ceil(n / 128) + E of them (n = T * topk), a workgroup walks offs (clamped into [0, n] and
//     made monotonic, so no plan can send a row outside the buffers) to its expert and row range and the tiles past
//     the last one exit at once.
//   * A (bf16) goes global -> LDS by LDS-DMA. Up: image row r is x[perm[row] / topk], the gather is the per-lane
//     source address; down: the contiguous sorted rows of h. Rows past the expert's end re-read its last row and are
//     never stored.
//   * B (codes): a lane loads 16 bytes of codes along K into registers two K tiles ahead of the MFMAs, turns them
//     into exact bf16 once (so once per weight element per workgroup, not once per M wave) and writes two 16-byte
//     chunks of the image. An int4 pair-row load feeds two image rows (low nibbles -> channel 2j, high -> 2j + 1),
//     so the int4 kernels issue one load per lane and K tile where the int8 kernels issue two. After the barrier the
//     loop is the bf16 grouped kernel's. The per-channel scale multiplies the finished fp32 sum in the epilogue.//   * tile fill: a wave whose 16-row fragments lie past the expert's end, or whose channels lie past a ragged band's
//     end, skips their LDS reads and MFMAs on a wave-uniform count; accumulators stay statically indexed.
//   * up: a band is 128 value channels [c0, c0 + 128) and their gates [f + c0, f + c0 + 128): image row
//     64 wn + 16 j + w holds channel c0 + 32 wn + 16 (j & 1) + w of the half j >> 1, so wave wn's fragments 0, 1 are
//     32 value channels and 2, 3 their gates. Epilogue on the accumulators: scale, b1, silu(value) * gate, one 8-byte
//     bf16 store of h [n, f] in sorted row order. Channels past f (f % 64 == 0: a band may hold 64) are clamped reads.
//   * down: a band is 256 channels of d (ragged alike), K = f. y [n, d] fp32 = sum * scale, every sorted row written
//     exactly once: no memset, no atomic. moe_decode_combine_k (moe_combine.h) with one slab adds b2, weights by val
//     and sums a token's experts in ascending order: the same bits every run.
//
// Limits (the launchers return 1 otherwise): 1 <= T <= 65535 (the combine's gridDim.y), E <= 256, topk <= min(8, E),
// d % 64 == f % 64 == 0, bits 8 or 4. Index arithmetic: n = T * topk <= 524280 and the launch's tile count
// (n / 128 + 1 + E) * bands fit 32 bits (checked); every row of x, h, y and of the code and scale tensors is
// addressed in 64 bits, so d and f have no further bound.
#include "common.h"
#include "launch.h"
#include "mfma_tile.h"
#include "moe_combine.h"
#include "wo_cvt.h"

namespace pa {
namespace {

constexpr int kGwTM = 128, kGwTN = 256;
constexpr int kGwMaxT = 65535, kGwMaxE = 256, kGwMaxTopk = 8;
constexpr int kGwAImg = kGwTM * 128, kGwStage = (kGwTM + kGwTN) * 128;  // bytes: a K tile is 64 bf16 = 128 B a row

struct MoeGwoArgs {
  const uint16_t* a;       // up: x [T, d]; down: h [n, f], sorted row order
  const uint8_t* bq;       // up: w1_q; down: w2_q
  const float* bs;         // up: w1_s [E, 2f]; down: w2_s [E, d]
  const uint16_t* b1;      // [E, 2f] bf16 or null (up)
  const int *offs, *perm;  // [E + 1]; [n] sorted row -> entry (up)
  uint16_t* h;             // up: [n, f] bf16, sorted row order
  float* y;                // down: [n, d] fp32, sorted row order
  int T, E, topk, d, f, n, tiles_n;
};

// One 128 x 256 tile of one expert. UP: A = x gathered through perm, B = value + gate channels of w1_q[e], epilogue
// scale + bias + SwiGLU -> h. !UP: A = sorted rows of h, B = w2_q[e], epilogue scale -> y.
template <int BITS, bool UP>
__global__ __launch_bounds__(512, 1) void moe_grouped_wo_k(MoeGwoArgs p) {
  constexpr int TM = kGwTM, TN = kGwTN;
  constexpr int MR = TM / 32, NR = 4;      // wave tile 64 x 64
  constexpr int NL = BITS == 8 ? 2 : 1;    // 16-byte code loads a lane makes per K tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  // tile map: the expert and the sorted rows [m0, mend) of M tile mt
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

  const int K = UP ? p.d : p.f, NC = UP ? p.f : p.d;  // reduction length; channels a band is cut from
  const int n0 = tn * (UP ? TN / 2 : TN);
  const uint8_t* bq = p.bq + (int64_t)e * ((UP ? 2 * p.f : p.d) / (8 / BITS)) * K;  // a code row is K bytes

  // the row maps: source row of A for tile row r; channel of the expert's B for image row r, clamped into the band's
  // matrix (int4: r even, clamped to an even channel, so r + 1 is its pair)
  auto a_row = [&](int r) {
    const int m = min(m0 + r, mend - 1);
    return UP ? min(max(p.perm[m] / p.topk, 0), p.T - 1) : m;
  };
  auto b_chan = [&](int r) {
    constexpr int last = BITS == 8 ? 1 : 2;
    if constexpr (UP) {
      const int j = (r >> 4) & 3;
      return (j >> 1) * p.f + min(n0 + (r >> 6) * 32 + 16 * (j & 1) + (r & 15), NC - last);
    } else {
      return min(n0 + r, NC - last);
    }
  };

  // A staging: wave-instruction q = 8 i + wave fills image rows 8 q + (lane >> 3), the lane's 16-byte chunk swizzled
  // by k_swz in its global source address
  const char* asrc[TM / 64];
#pragma unroll
  for (int i = 0; i < TM / 64; ++i) {
    const int row = (i * 8 + wave) * 8 + (lane >> 3);
    asrc[i] = reinterpret_cast<const char*>(p.a + (int64_t)a_row(row) * K) + (((lane & 7) ^ k_swz(row)) << 4);
  }
  // B staging: load l of thread tid is the 16 codes k = 16 part .. 16 part + 15 of image row brow[l] (int4: of rows
  // brow[0] and brow[0] + 1), which are the image chunks 2 part and 2 part + 1
  const uint8_t* bsrc[NL];
  int bdst[NL][2];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int idx = l * 512 + tid, part = idx & 3;
    const int row = BITS == 8 ? idx >> 2 : 2 * (idx >> 2);
    bsrc[l] = bq + (int64_t)(b_chan(row) / (8 / BITS)) * K + part * 16;
    bdst[l][0] = kGwAImg + row * 128 + (((2 * part) ^ k_swz(row)) << 4);
    bdst[l][1] = kGwAImg + row * 128 + (((2 * part + 1) ^ k_swz(row)) << 4);
  }
  const int nk = K / 64;
  uint4 raw[NL];
  auto load_b = [&](int t) {
#pragma unroll
    for (int l = 0; l < NL; ++l) raw[l] = *reinterpret_cast<const uint4*>(bsrc[l] + (int64_t)t * 64);
  };
  auto stage_a = [&](int t, int buf) {
#pragma unroll
    for (int i = 0; i < TM / 64; ++i) glds16(asrc[i] + (int64_t)t * 128, smem + buf * kGwStage + (i * 8 + wave) * 1024);
  };
  auto stage_b = [&](int buf) {  // raw -> bf16 -> image
    char* base = smem + buf * kGwStage;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      uint4 c0, c1;
      gwo_cvt<BITS, false>(raw[l], c0, c1);
      *reinterpret_cast<uint4*>(base + bdst[l][0]) = c0;
      *reinterpret_cast<uint4*>(base + bdst[l][1]) = c1;
      if constexpr (BITS == 4) {  // the odd channel of the pair: the next image row, the same swizzle (row is even)
        gwo_cvt<4, true>(raw[l], c0, c1);
        *reinterpret_cast<uint4*>(base + bdst[l][0] + 128) = c0;
        *reinterpret_cast<uint4*>(base + bdst[l][1] + 128) = c1;
      }
    }
  };

  // 16-row fragments of this wave that hold rows of the expert; none when the wave's channels lie past the band's end
  // (whole waves: NC % 64 == 0 and a wave owns 32 (up) or 64 (down) channels)
  const int wcol = n0 + wn * (UP ? 32 : 64);
  const int nfr = wcol < NC ? min(max((mend - m0 - wm * (TM / 2) + 15) >> 4, 0), MR) : 0;

  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // The code registers run two K tiles ahead of the MFMAs, the LDS image one. Every step issues its LDS-DMA before its
  // code loads, so vmcnt(NL) retires the DMA and leaves the code loads in flight across the barrier.
  load_b(0);
  stage_a(0, 0);
  stage_b(0);
  load_b(min(1, nk - 1));
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NL) : "memory");
  bar();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk) {
      stage_b(cur ^ 1);  // tile t + 1, loaded a step ago
      stage_a(t + 1, cur ^ 1);
      load_b(min(t + 2, nk - 1));
    }
    const char* aimg = smem + cur * kGwStage;
    const char* bimg = aimg + kGwAImg;
    // a full wave tile runs the bf16 kernel's straight-line body; a partial one tests each fragment
    auto mma = [&](auto full) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8_t bf[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) bf[j] = frag<TN, true>(bimg, wn * 64 + j * 16, s, lane);
#pragma unroll
        for (int i = 0; i < MR; ++i) {
          if (!decltype(full)::value && i >= nfr) continue;
          const bf16x8_t af = frag<TM, true>(aimg, wm * (TM / 2) + i * 16, s, lane);
#pragma unroll
          for (int j = 0; j < NR; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af, acc[i][j], 0, 0, 0);
        }
      }
    };
    if (nfr == MR) mma(IntC<1>{});
    else if (nfr > 0) mma(IntC<0>{});
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NL) : "memory");
    bar();
  }
  if (nfr == 0) return;

  // lane holds, of sorted row mrow0 + 16 i, the accumulator columns 64 wn + 16 j + 4 g + 0..3
  const int g = lane >> 4;
  const int mrow0 = m0 + wm * (TM / 2) + (lane & 15);
  if constexpr (UP) {
    // columns 16 j + 4 g + q of fragments j = 0, 1 are value channels wcol + 16 j + 4 g + q, of j = 2, 3 their gates
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = wcol + 16 * j + 4 * g;
      const float* sp = p.bs + (int64_t)e * 2 * p.f + c;
      const float4 sa = *reinterpret_cast<const float4*>(sp), sg = *reinterpret_cast<const float4*>(sp + p.f);
      const float sav[4] = {sa.x, sa.y, sa.z, sa.w}, sgv[4] = {sg.x, sg.y, sg.z, sg.w};
      float ba[4] = {0.f, 0.f, 0.f, 0.f}, bg[4] = {0.f, 0.f, 0.f, 0.f};
      if (p.b1) {
        const uint16_t* b = p.b1 + (int64_t)e * 2 * p.f + c;
        load4_16(b, ba);
        load4_16(b + p.f, bg);
      }
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int m = mrow0 + i * 16;
        if (i >= nfr || m >= mend) continue;
        float h[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          h[q] = silu(acc[i][j][q] * sav[q] + ba[q]) * (acc[i][2 + j][q] * sgv[q] + bg[q]);
        *reinterpret_cast<uint2*>(p.h + (int64_t)m * p.f + c) = make_uint2(pack_bf16(h[0], h[1]), pack_bf16(h[2], h[3]));
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int c = wcol + 16 * j + 4 * g;
      const float4 s = *reinterpret_cast<const float4*>(p.bs + (int64_t)e * p.d + c);
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int m = mrow0 + i * 16;
        if (i >= nfr || m >= mend) continue;
        *reinterpret_cast<float4*>(p.y + (int64_t)m * p.d + c) =
            make_float4(acc[i][j][0] * s.x, acc[i][j][1] * s.y, acc[i][j][2] * s.z, acc[i][j][3] * s.w);
      }
    }
  }
}

bool moe_grouped_wo_shape_ok(int T, int E, int topk, int d, int f, int bits) {
  return T >= 1 && T <= kGwMaxT && E >= 1 && E <= kGwMaxE && topk >= 1 && topk <= kGwMaxTopk && topk <= E &&
         d >= 64 && f >= 64 && d % 64 == 0 && f % 64 == 0 && (bits == 8 || bits == 4);
}

template <bool UP>
int launch_grouped_wo(MoeGwoArgs& p, int bits, hipStream_t st) {
  p.tiles_n = UP ? (p.f + kGwTN / 2 - 1) / (kGwTN / 2) : (p.d + kGwTN - 1) / kGwTN;
  const int64_t grid = (int64_t)((p.n + kGwTM - 1) / kGwTM + p.E) * p.tiles_n;
  if (grid >= (1ll << 31)) return 1;
  const dim3 g((unsigned)grid), b(512);
  constexpr int lds = 2 * kGwStage;
  return bits == 8 ? launch_lds<moe_grouped_wo_k<8, UP>>(g, b, lds, st, p)
                   : launch_lds<moe_grouped_wo_k<4, UP>>(g, b, lds, st, p);
}

}  // namespace
}  // namespace pa

using namespace pa;

// Up projection of the weight-only expert FFN over expert-sorted rows: x [T, d] bf16, w1q [E, 2f, d] int8 (bits 8) or
// [E, f, d] int4 pair-rows (bits 4), w1s [E, 2f] fp32, b1 [E, 2f] bf16 or null, offs [E + 1] and perm [n] int32 as
// pa_moe_route leaves them (n = T * topk entries, all kept) -> h [n, f] bf16 = silu(value) * gate in sorted row order
// (needs no clearing). Returns 1 for a shape it does not take (the limits at the top of this file).
PA_EXPORT int pa_moe_grouped_up_wo(const void* x, const void* w1q, const float* w1s, const void* b1, const int* offs,
                                   const int* perm, void* h, int T, int E, int topk, int d, int f, int bits,
                                   hipStream_t st) {
  if (!moe_grouped_wo_shape_ok(T, E, topk, d, f, bits)) return 1;
  MoeGwoArgs p{};
  p.a = (const uint16_t*)x; p.bq = (const uint8_t*)w1q; p.bs = w1s; p.b1 = (const uint16_t*)b1;
  p.offs = offs; p.perm = perm; p.h = (uint16_t*)h;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk;
  return launch_grouped_wo<true>(p, bits, st);
}

// Down projection and combine: h as pa_moe_grouped_up_wo leaves it, w2q [E, d, f] int8 or [E, d / 2, f] int4
// pair-rows, w2s [E, d] fp32, b2 [E, d] bf16 or null, val [T, topk] fp32, idx [T, topk] and pos [n] (entry -> sorted
// row) int32, y = n * d fp32 of workspace (need not be cleared) -> out [T, d] bf16. Returns 1 for a shape it does not
// take.
PA_EXPORT int pa_moe_grouped_down_wo(const void* h, const void* w2q, const float* w2s, const void* b2,
                                     const float* val, const int* idx, const int* offs, const int* pos, float* y,
                                     void* out, int T, int E, int topk, int d, int f, int bits, hipStream_t st) {
  if (!moe_grouped_wo_shape_ok(T, E, topk, d, f, bits)) return 1;
  MoeGwoArgs p{};
  p.a = (const uint16_t*)h; p.bq = (const uint8_t*)w2q; p.bs = w2s; p.offs = offs; p.y = y;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk;
  const int rc = launch_grouped_wo<false>(p, bits, st);
  if (rc) return rc;
  MoeDecArgs c{};
  c.b2 = (const uint16_t*)b2; c.val = val; c.idx = idx; c.pos = pos; c.ws = y; c.out = (uint16_t*)out;
  c.T = T; c.E = E; c.topk = topk; c.d = d; c.f = f; c.n = p.n; c.splits = 1;
  hipLaunchKernelGGL(moe_decode_combine_k, dim3((d / 4 + 255) / 256, T), dim3(256), 0, st, c);
  return (int)hipGetLastError();
}
