// MoE decode: the SwiGLU expert FFN of fused_moe for at most 64 tokens (serving), as four launches with no host
// synchronisation: plan -> up projection (+ SwiGLU) -> down projection (K split) -> combine.
// Reference behaviour: python/paddle/incubate/nn/functional/fused_moe.py:20 (softmax gate, top-k, optional
// renormalisation, ffn1 [E, d, 2f] -> swiglu -> ffn2 [E, f, d], weighted sum over the token's experts).
//
// Decode MoE is bound by the bytes of the routed experts' weights, so the two projections are built like the dense
// decode GEMM (gemm.hip gemm_small_m_kernel): few rows, a 4-deep LDS ring filled by LDS-DMA, one barrier per K
// tile, counted vmcnt waits. What is this file's own:
//   * moe_decode_plan_k, one workgroup: softmax + top-k + renormalisation per token (one wave per token), then a
//     stable counting sort of the T * topk entries held in LDS. A token picks an expert at most once, so an expert
//     holds at most T <= 64 rows = one M tile: the ascending list of non-empty experts IS the tile map, and the
//     GEMM grids are (column bands) x (slots), a slot past the active count exiting at once.
//   * the row-gather stage: the A operand of the up projection is not a gathered copy of x; the token index
//     perm[row] / topk goes into the per-lane LDS-DMA source address. Rows past the expert's count are clamped
//     reads that are never stored.
//   * the up projection stages the value band [n0, n0 + 64) and the gate band [f + n0, f + n0 + 64) of w1[e] side
//     by side, so bias + silu(value) * gate happens on the accumulators and h [n, f] is written once, in bf16.
//   * the down projection splits K over gridDim.z into fp32 slabs [split][n][d]; every row of every slab is
//     written (each sorted row belongs to exactly one expert), so there is no memset and no atomic.
//   * moe_decode_combine_k (moe_combine.h, shared with moe_grouped_mx.hip) sums slabs, bias and the token's experts
//     in a fixed ascending order: bit-identical from run to run.
//
// MXFP4 expert weights (pa_moe_decode_up_mx / pa_moe_decode_down_mx; formats in mx.hip): the same plan and the same
// combine around two projections built like mx.hip's gemm_mx_small_m_k instead of the LDS ring, since 4.25-bit weights
// leave nothing to stage: w1_q [E, 2f, d / 2] and w2_q [E, d, f / 2] are K-major per expert, a lane's 16-byte weight
// fragment and its E8M0 byte go from global memory into v_mfma_scale_f32_16x16x128_f8f6f4 two of its wave's steps
// ahead, the four waves interleave the 128-k steps and their sums meet in LDS in wave order. Activations are mxfp8 at
// both projections: x is quantised once by pa_mx_quant ([T, d] codes + [T, d / 32] scales) and gathered through
// perm[row] / topk in the lane's pointers; the up kernel owns 32 value channels and the 32 gate channels f + n, one
// 32-block of h, so bias + silu(value) * gate, the block's amax, its E8M0 byte and the e4m3 codes (mx_block.h, the
// quantiser's own rule) all happen in its epilogue and h exists only as h_q [n, f] + h_s [n, f / 32]. The loop over
// 16-row fragments runs to ceil(cnt / 16) of the expert's own count (uniform in the workgroup), not to a template
// parameter from T: at 64 tokens over many experts most experts hold one or two rows. The accumulators stay
// statically indexed (unrolled over 4, skipped on the uniform predicate). The down projection splits K = f over
// gridDim.z in whole 128-k steps into the same fp32 slabs, which moe_decode_combine_k sums.
//   Deviations from the plain sketch: the cross-wave reduction runs one row fragment at a time through a 16-KiB (up)
// / 8-KiB (down) buffer instead of holding all four fragments (64 KiB) at once; it costs two barriers per live
// fragment and keeps LDS out of what limits occupancy (registers do: 2 waves a SIMD up, 3 down).
#include "launch.h"
#include "mfma_tile.h"
#include "moe_combine.h"
#include "mx_block.h"

namespace pa {
namespace {

constexpr int kMdBK = 64, kMdBN = 64, kMdNW = 4, kMdStages = 4;
constexpr int kMdMaxT = 64, kMdMaxE = 256, kMdMaxTopk = 8, kMdMaxN = kMdMaxT * kMdMaxTopk;

// ------------------------------------------------------------------------------------------------ plan
// logits [T, E] -> val / idx [T, topk], offs [E + 1], perm [n] (sorted row -> entry, stable), pos [n] (entry ->
// sorted row), active [min(E, n)] (non-empty experts ascending, -1 behind them), n_active [1].  n = T * topk.
template <class TL>
__global__ __launch_bounds__(256) void moe_decode_plan_k(const TL* __restrict__ logits, int T, int E, int topk,
                                                         int norm, float* __restrict__ val, int* __restrict__ idx,
                                                         int* __restrict__ offs, int* __restrict__ perm,
                                                         int* __restrict__ pos, int* __restrict__ active,
                                                         int* __restrict__ n_active) {
  __shared__ float s_val[kMdMaxN];
  __shared__ int s_idx[kMdMaxN], s_rank[kMdMaxN], s_offs[kMdMaxE], s_wtot[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = T * topk;

  // gate: lane holds experts lane, lane + 64, lane + 128, lane + 192
  for (int t = wave; t < T; t += 4) {
    float p[4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      p[i] = c < E ? to_f(logits[(int64_t)t * E + c]) : -INFINITY;
      mx = fmaxf(mx, p[i]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = lane + 64 * i < E ? expf(p[i] - mx) : 0.f;
      sum += p[i];
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = p[i] / sum;
      if (!(p[i] >= 0.f)) p[i] = 0.f;           // NaN logits: still topk distinct experts
      if (lane + 64 * i >= E) p[i] = -2.f;      // never picked: topk <= E
    }
    // topk rounds of (largest value, lowest index); a picked expert drops to -1
    float tot = 0.f, myv = 0.f;
    int myi = 0;
    for (int j = 0; j < topk; ++j) {
      float bv = -3.f;
      int bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p[i] > bv) { bv = p[i]; bi = lane + 64 * i; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i == bi) p[i] = -1.f;
      if (lane == j) { myv = bv; myi = bi; }
      tot += bv;
    }
    if (lane < topk) {
      s_val[t * topk + lane] = norm ? myv / tot : myv;
      s_idx[t * topk + lane] = myi;
    }
  }
  __syncthreads();

  // stable counting sort: thread e walks the entries in order and numbers its own
  int c = 0;
  if (tid < E)
    for (int j = 0; j < n; ++j)
      if (s_idx[j] == tid) s_rank[j] = c++;
  // one exclusive scan for both the row offsets (low half) and the active-list slots (high half); n <= 512
  const int v = c | ((c > 0) << 16);
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) s_wtot[wave] = inc;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) base += s_wtot[w];
    total += s_wtot[w];
  }
  const int exc = base + inc - v;
  const int n_act = total >> 16, slots = E < n ? E : n;
  if (tid < E) {
    s_offs[tid] = exc & 0xffff;
    offs[tid] = exc & 0xffff;
    if (c > 0) active[exc >> 16] = tid;
  }
  if (tid >= n_act && tid < slots) active[tid] = -1;
  if (tid == 0) {
    offs[E] = total & 0xffff;
    *n_active = n_act;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int e = s_idx[i];
    const int r = s_offs[e] + s_rank[i];
    pos[i] = r;
    perm[r] = i;
    val[i] = s_val[i];
    idx[i] = e;
  }
}

// ------------------------------------------------------------------------------------------------ FFN
// One tile of one active expert: C[rows of e (<= MT * 16), 64 columns] over nk K tiles.
//   UP:  A = x gathered through perm, B = the value and the gate band of w1[e]; epilogue bias + swiglu -> h (bf16)
//   !UP: A = rows of h,              B = one band of w2[e], K range of split blockIdx.z;   epilogue fp32 slab
// 4 waves, wave w owns columns [16 w, 16 w + 16) of the band(s) for all MT row fragments. Ring of kMdStages stages of
// A ([AR][64] K-major, swizzled) + NB B images ([64 k][64] MN-major): 20-24 KiB a stage for UP, 12-16 KiB for down.
template <int MT, bool UP>
__device__ __forceinline__ void moe_decode_tile(const MoeDecArgs& p) {
  constexpr int AR = MT <= 2 ? 32 : 64;  // staged A rows: one or two 1-KiB LDS-DMA instructions per thread
  constexpr int NQA = AR / (8 * kMdNW), NB = UP ? 2 : 1;
  constexpr int A_BYTES = AR * kMdBK * 2, B_BYTES = kMdBN * kMdBK * 2, STAGE = A_BYTES + NB * B_BYTES;
  constexpr int NL = NQA + NB * (kMdBN / (8 * kMdNW));  // glds per thread per K tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int slot = blockIdx.y;
  if (slot >= *p.n_active) return;
  const int e = p.active[slot];
  if ((unsigned)e >= (unsigned)p.E) return;
  const int r0 = p.offs[e];
  const int cnt = min(min(p.offs[e + 1] - r0, MT * 16), p.n - r0);
  if (r0 < 0 || cnt <= 0) return;
  const int n0 = blockIdx.x * kMdBN;
  const int K = UP ? p.d : p.f, ldb = UP ? 2 * p.f : p.d;
  const int kbeg = UP ? 0 : blockIdx.z * p.k_per;
  const int nk = (UP ? p.d : p.k_per) / kMdBK;
  const uint16_t* bw = (UP ? p.w1 : p.w2) + (int64_t)e * p.d * p.f * (UP ? 2 : 1);

  // row-gather stage: the source row of every image row this lane fills, swizzled chunk included
  const uint16_t* arow[NQA];
#pragma unroll
  for (int i = 0; i < NQA; ++i) {
    const int row = (i * kMdNW + wave) * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ k_swz(row);
    const int rr = r0 + min(row, cnt - 1);
    int src = rr;
    if (UP) src = min(max(p.perm[rr] / p.topk, 0), p.T - 1);
    arow[i] = (UP ? p.x : p.h) + (int64_t)src * K + kbeg + lc * 8;
  }
  auto stage_tile = [&](int t) {
    char* base = smem + (t % kMdStages) * STAGE;
#pragma unroll
    for (int i = 0; i < NQA; ++i) glds16(arow[i] + t * kMdBK, base + (i * kMdNW + wave) * 1024);
    stage<kMdBN, false, kMdNW>(bw, ldb, n0, ldb, kbeg + t * kMdBK, base + A_BYTES, wave, lane);
    if (UP) stage<kMdBN, false, kMdNW>(bw, ldb, p.f + n0, ldb, t * kMdBK, base + A_BYTES + B_BYTES, wave, lane);
  };

  f32x4 acc[MT][NB];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int pro = min(kMdStages - 1, nk);
  for (int t = 0; t < pro; ++t) stage_tile(t);
  // wait for tile 0: (pro - 1) tiles may stay in flight
  if (pro >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL) : "memory");
  else if (pro == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  bar();

#pragma unroll 1
  for (int t = 0; t < nk; ++t) {
    if (t + kMdStages - 1 < nk) stage_tile(t + kMdStages - 1);
    const char* aimg = smem + (t % kMdStages) * STAGE;
    const char* bimg = aimg + A_BYTES;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8_t bf[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) bf[j] = frag<kMdBN, false>(bimg + j * B_BYTES, wave * 16, s, lane);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const bf16x8_t af = frag<AR, true>(aimg, i * 16, s, lane);
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af, acc[i][j], 0, 0, 0);
      }
    }
    // retire tile t + 1 (tiles issued after it may stay in flight)
    const int after = min(nk - 1, t + kMdStages - 1) - (t + 1);
    if (after >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL) : "memory");
    else if (after == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar();
  }

  // lane holds C[m = 16 i + (lane & 15)][n0 + 16 wave + 4 (lane >> 4) + 0..3]
  const int col = n0 + wave * 16 + 4 * (lane >> 4);
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = i * 16 + (lane & 15);
    if (m >= cnt) continue;
    if constexpr (UP) {
      float a[4] = {acc[i][0][0], acc[i][0][1], acc[i][0][2], acc[i][0][3]};
      float g[4] = {acc[i][1][0], acc[i][1][1], acc[i][1][2], acc[i][1][3]};
      if (p.b1) {
        float ba[4], bg[4];
        load4_16(p.b1 + (int64_t)e * 2 * p.f + col, ba);
        load4_16(p.b1 + (int64_t)e * 2 * p.f + p.f + col, bg);
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] += ba[q]; g[q] += bg[q]; }
      }
      *reinterpret_cast<uint2*>(p.h + (int64_t)(r0 + m) * p.f + col) =
          make_uint2(pack_bf16(silu(a[0]) * g[0], silu(a[1]) * g[1]), pack_bf16(silu(a[2]) * g[2], silu(a[3]) * g[3]));
    } else {
      *reinterpret_cast<float4*>(p.ws + ((int64_t)blockIdx.z * p.n + r0 + m) * p.d + col) =
          make_float4(acc[i][0][0], acc[i][0][1], acc[i][0][2], acc[i][0][3]);
    }
  }
}

template <int MT>
__global__ __launch_bounds__(kMdNW * 64) void moe_decode_up_k(MoeDecArgs p) { moe_decode_tile<MT, true>(p); }
template <int MT>
__global__ __launch_bounds__(kMdNW * 64) void moe_decode_down_k(MoeDecArgs p) { moe_decode_tile<MT, false>(p); }

template <int MT, bool UP>
constexpr int moe_decode_smem() {
  return kMdStages * ((MT <= 2 ? 32 : 64) * kMdBK * 2 + (UP ? 2 : 1) * kMdBN * kMdBK * 2);
}

bool moe_decode_shape_ok(int T, int E, int topk, int d, int f) {
  return T >= 1 && T <= kMdMaxT && E >= 1 && E <= kMdMaxE && topk >= 1 && topk <= kMdMaxTopk && topk <= E &&
         d >= kMdBK && f >= kMdBK && d % 64 == 0 && f % 64 == 0;
}

// ------------------------------------------------------------------------------------------------ MXFP4 experts
struct MoeDecMxArgs {
  const uint8_t *xq, *xs;    // [T, d] e4m3fn, [T, d / 32]
  const uint8_t *w1q, *w1s;  // [E, 2f, d / 2] e2m1 pairs, [E, 2f, d / 32]
  const uint8_t *w2q, *w2s;  // [E, d, f / 2], [E, d, f / 32]
  const uint16_t* b1;        // [E, 2f] bf16 or null
  const int *offs, *perm, *active, *n_active;
  uint8_t *hq, *hs;          // [n, f] e4m3fn, [n, f / 32], sorted row order
  float* ws;                 // [splits, n, d] fp32
  int T, E, topk, d, f, n, steps_per;
};

constexpr int kMxBand = 32;  // channels of a workgroup's band: one 32-block of h in the up projection

// the expert of this slot and its sorted rows [r0, r0 + cnt); false for a slot with nothing to do or a plan that
// does not fit the buffers
__device__ __forceinline__ bool moe_mx_slot(const MoeDecMxArgs& p, int slot, int& e, int& r0, int& cnt) {
  if (slot >= *p.n_active) return false;
  e = p.active[slot];
  if ((unsigned)e >= (unsigned)p.E) return false;
  r0 = p.offs[e];
  if (r0 < 0 || r0 >= p.n) return false;
  cnt = min(min(p.offs[e + 1] - r0, kMdMaxT), p.n - r0);
  return cnt > 0;
}

// The K loop of both projections: this wave's 128-k steps wave, wave + 4, ... of nst. wrow / wsc: the lane's weight
// row (channel lane & 15 of each 16-channel tile) and its scale bytes at k-group lane >> 4 of step 0; arow / asc: the
// same for the lane's mxfp8 activation row of each 16-row fragment. The weight stream, the only operand that comes
// from HBM, runs two of the wave's steps ahead of the MFMAs; the activations are L2 hits. Fragments past nfrag
// (wave-uniform) are skipped, the accumulators stay statically indexed.
template <int NT>
__device__ __forceinline__ void moe_mx_stream(const uint8_t* const (&wrow)[NT], const uint8_t* const (&wsc)[NT],
                                              const uint8_t* const (&arow)[4], const uint8_t* const (&asc)[4],
                                              int nfrag, int nst, int wave, f32x4 (&acc)[4][NT]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 raw0[NT], raw1[NT];
  int s0[NT], s1[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const bool h0 = wave < nst, h1 = wave + 4 < nst;
    raw0[j] = h0 ? *reinterpret_cast<const uint4*>(wrow[j] + wave * 64) : make_uint4(0, 0, 0, 0);
    s0[j] = h0 ? (int)wsc[j][wave * 4] : 127;
    raw1[j] = h1 ? *reinterpret_cast<const uint4*>(wrow[j] + (wave + 4) * 64) : make_uint4(0, 0, 0, 0);
    s1[j] = h1 ? (int)wsc[j][(wave + 4) * 4] : 127;
  }
  for (int c = wave; c < nst; c += 4) {
    i32x8 bf[NT];
    int bs[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bf[j] = widen(raw0[j]);
      bs[j] = s0[j];
      raw0[j] = raw1[j];
      s0[j] = s1[j];
      const bool h = c + 8 < nst;
      raw1[j] = h ? *reinterpret_cast<const uint4*>(wrow[j] + (int64_t)(c + 8) * 64) : make_uint4(0, 0, 0, 0);
      s1[j] = h ? (int)wsc[j][(c + 8) * 4] : 127;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= nfrag) continue;
      const uint8_t* ap = arow[t] + (int64_t)c * 128;
      const i32x8 af = join(*reinterpret_cast<const uint4*>(ap), *reinterpret_cast<const uint4*>(ap + 64));
      const int as = (int)asc[t][c * 4];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[t][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf[j], acc[t][j], kFmtFp8, kFmtFp4, 0, as, 0,
                                                                     bs[j]);
    }
  }
}

// one fragment's partial sums of this wave into red[wave]: tile j at j * 256, [16 rows][16 channels]. The MFMA leaves
// channel lane & 15 and rows 4 (lane >> 4) + r in the lane.
template <int NT>
__device__ __forceinline__ void moe_mx_put(float (&red)[4][NT * 256], const f32x4 (&a)[NT], int wave, int lane) {
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][j * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)] = a[j][r];
}
template <int NT>
__device__ __forceinline__ float moe_mx_sum(const float (&red)[4][NT * 256], int i) {
  return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// Up projection + SwiGLU + mxfp8 quantisation of h. grid (f / 32, slots). Tiles 0, 1: value channels [n0, n0 + 32);
// tiles 2, 3: gate channels [f + n0, f + n0 + 32).
__global__ __launch_bounds__(256) void moe_decode_up_mx_k(MoeDecMxArgs p) {
  constexpr int NT = 4;
  __shared__ float red[4][NT * 256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, g = lane >> 4;
  int e, r0, cnt;
  if (!moe_mx_slot(p, blockIdx.y, e, r0, cnt)) return;
  const int n0 = blockIdx.x * kMxBand, nfrag = (cnt + 15) >> 4;
  const int ldq = p.d / 2, lds = p.d / 32;
  const uint8_t* wrow[NT];
  const uint8_t* wsc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int64_t ch = (int64_t)e * 2 * p.f + (j < 2 ? n0 + j * 16 : p.f + n0 + (j - 2) * 16) + col;
    wrow[j] = p.w1q + ch * ldq + g * 16;
    wsc[j] = p.w1s + ch * lds + g;
  }
  // row gather: the token of the lane's row of each fragment; rows past the count are clamped reads, never stored
  const uint8_t* arow[4];
  const uint8_t* asc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int m = min(t * 16 + col, cnt - 1);
    const int tok = min(max(p.perm[r0 + m] / p.topk, 0), p.T - 1);
    arow[t] = p.xq + (int64_t)tok * p.d + g * 16;
    asc[t] = p.xs + (int64_t)tok * lds + g;
  }
  f32x4 acc[4][NT];
  moe_mx_stream<NT>(wrow, wsc, arow, asc, nfrag, p.d / 128, wave, acc);

  // epilogue, a fragment at a time: thread -> row tid >> 4 of the fragment, channels 2 (tid & 15) + {0, 1} of the
  // band; the row's 32-block is the 16 lanes of one DPP row
  const int ml = tid >> 4, c2 = (tid & 15) * 2;
  float ba[2] = {0.f, 0.f}, bg[2] = {0.f, 0.f};
  if (p.b1) {
    const uint16_t* b = p.b1 + (int64_t)e * 2 * p.f + n0 + c2;
    const uint32_t va = *reinterpret_cast<const uint32_t*>(b), vg = *reinterpret_cast<const uint32_t*>(b + p.f);
    ba[0] = lo_bf16(va); ba[1] = hi_bf16(va); bg[0] = lo_bf16(vg); bg[1] = hi_bf16(vg);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nfrag) continue;
    moe_mx_put<NT>(red, acc[t], wave, lane);
    __syncthreads();
    float h[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = ((c2 + q) >> 4) * 256 + ml * 16 + ((c2 + q) & 15);
      const float a = moe_mx_sum<NT>(red, i) + ba[q], gt = moe_mx_sum<NT>(red, i + 512) + bg[q];
      h[q] = silu(a) * gt;
    }
    float amax = fmaxf(fabsf(h[0]), fabsf(h[1]));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const int eb = mx_block_exp<8>(amax);
    const uint32_t code = mx_e4m3x2<false>(h[0], h[1], mx_block_mult(eb), 0);
    const int m = t * 16 + ml;
    if (m < cnt) {
      *reinterpret_cast<uint16_t*>(p.hq + (int64_t)(r0 + m) * p.f + n0 + c2) = (uint16_t)(code & 0xffffu);
      if ((tid & 15) == 0) p.hs[(int64_t)(r0 + m) * (p.f / 32) + blockIdx.x] = (uint8_t)eb;
    }
    __syncthreads();
  }
}

// Down projection: rows of h_q x one 32-channel band of w2_q[e] over the 128-k steps of split blockIdx.z -> fp32
// slab. grid (d / 32, slots, splits).
__global__ __launch_bounds__(256) void moe_decode_down_mx_k(MoeDecMxArgs p) {
  constexpr int NT = 2;
  __shared__ float red[4][NT * 256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, g = lane >> 4;
  int e, r0, cnt;
  if (!moe_mx_slot(p, blockIdx.y, e, r0, cnt)) return;
  const int n0 = blockIdx.x * kMxBand, nfrag = (cnt + 15) >> 4;
  const int step0 = blockIdx.z * p.steps_per, nst = min(p.steps_per, p.f / 128 - step0);
  const int ldq = p.f / 2, lds = p.f / 32;
  const uint8_t* wrow[NT];
  const uint8_t* wsc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int64_t ch = (int64_t)e * p.d + n0 + j * 16 + col;
    wrow[j] = p.w2q + ch * ldq + (int64_t)step0 * 64 + g * 16;
    wsc[j] = p.w2s + ch * lds + step0 * 4 + g;
  }
  const uint8_t* arow[4];
  const uint8_t* asc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t row = r0 + min(t * 16 + col, cnt - 1);
    arow[t] = p.hq + row * p.f + (int64_t)step0 * 128 + g * 16;
    asc[t] = p.hs + row * lds + step0 * 4 + g;
  }
  f32x4 acc[4][NT];
  moe_mx_stream<NT>(wrow, wsc, arow, asc, nfrag, nst, wave, acc);

  float* slab = p.ws + ((int64_t)blockIdx.z * p.n + r0) * p.d + n0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nfrag) continue;
    moe_mx_put<NT>(red, acc[t], wave, lane);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {  // thread -> rows (tid >> 5) + 8 q, channel tid & 31: a row's band is 128 bytes
      const int ml = (tid >> 5) + 8 * q, c = tid & 31, m = t * 16 + ml;
      const float v = moe_mx_sum<NT>(red, (c >> 4) * 256 + ml * 16 + (c & 15));
      if (m < cnt) slab[(int64_t)m * p.d + c] = v;
    }
    __syncthreads();
  }
}

bool moe_decode_mx_shape_ok(int T, int E, int topk, int d, int f) {
  return moe_decode_shape_ok(T, E, topk, d, f) && d % 128 == 0 && f % 128 == 0;
}

}  // namespace
}  // namespace pa

using namespace pa;

// Gate + routing of a decode step: logits [T, E] (dtype 0 = fp32, 2 = bf16), T <= 64, E <= 256, topk <= min(8, E).
PA_EXPORT int pa_moe_decode_plan(const void* logits, int dtype, int T, int E, int topk, int norm, float* val, int* idx,
                                 int* offs, int* perm, int* pos, int* active, int* n_active, hipStream_t st) {
  if (T < 1 || T > kMdMaxT || E < 1 || E > kMdMaxE || topk < 1 || topk > kMdMaxTopk || topk > E) return 1;
  if (dtype == kF32)
    hipLaunchKernelGGL(moe_decode_plan_k<float>, dim3(1), dim3(256), 0, st, (const float*)logits, T, E, topk, norm,
                       val, idx, offs, perm, pos, active, n_active);
  else if (dtype == kBF16)
    hipLaunchKernelGGL(moe_decode_plan_k<bf16>, dim3(1), dim3(256), 0, st, (const bf16*)logits, T, E, topk, norm, val,
                       idx, offs, perm, pos, active, n_active);
  else
    return 2;
  return (int)hipGetLastError();
}

// K splits of the down projection the FFN runs with by default: the smallest divisor of f / 64 (at most 8, at least
// 8 K tiles a split) that gives every compute unit two workgroups if all min(E, n) slots are active.
PA_EXPORT int pa_moe_decode_splits(int n, int E, int d, int f) {
  if (n < 1 || E < 1 || d < 64 || f < 64) return 1;
  const int64_t wgs = (int64_t)(d / kMdBN) * (E < n ? E : n), target = 2 * device_cus();
  const int tiles = f / kMdBK;
  int s = 1;
  for (int c = 1; c <= 8 && tiles / c >= 8; ++c) {
    if (tiles % c) continue;
    s = c;
    if (wgs * c >= target) break;
  }
  return s;
}

// The expert FFN on a plan of pa_moe_decode_plan: x [T, d], w1 [E, d, 2f], w2 [E, f, d], b1 [E, 2f] / b2 [E, d] or
// null, all bf16 and contiguous; h = n * f bf16 and ws = splits * n * d fp32 of workspace (n = T * topk, neither needs
// clearing); out [T, d] bf16. d % 64 == 0, f % 64 == 0, (f / 64) % splits == 0.
PA_EXPORT int pa_moe_decode_ffn(const void* x, const void* w1, const void* w2, const void* b1, const void* b2,
                                const float* val, const int* idx, const int* offs, const int* perm, const int* pos,
                                const int* active, const int* n_active, void* h, float* ws, void* out, int T, int E,
                                int topk, int d, int f, int splits, hipStream_t st) {
  if (!moe_decode_shape_ok(T, E, topk, d, f)) return 1;
  if (splits < 1 || (f / kMdBK) % splits != 0) return 2;
  MoeDecArgs p{(const uint16_t*)x, (const uint16_t*)w1, (const uint16_t*)w2, (const uint16_t*)b1, (const uint16_t*)b2,
               val, idx, offs, perm, pos, active, n_active, (uint16_t*)h, ws, (uint16_t*)out,
               T, E, topk, d, f, T * topk, f / splits, splits};
  const int slots = E < p.n ? E : p.n;
  const dim3 block(kMdNW * 64), gup(f / kMdBN, slots), gdn(d / kMdBN, slots, splits);
  const auto run = [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    const int rc = launch_lds<moe_decode_up_k<MT>>(gup, block, moe_decode_smem<MT, true>(), st, p);
    return rc ? rc : launch_lds<moe_decode_down_k<MT>>(gdn, block, moe_decode_smem<MT, false>(), st, p);
  };
  const int mt = (T + 15) / 16;
  const int rc = mt == 1 ? run(IntC<1>{}) : mt == 2 ? run(IntC<2>{}) : mt == 3 ? run(IntC<3>{}) : run(IntC<4>{});
  if (rc) return rc;
  hipLaunchKernelGGL(moe_decode_combine_k, dim3((d / 4 + 255) / 256, T), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// K splits of the MXFP4 down projection by default: the fewest (at most 8, at least two 128-k steps each) that give
// every compute unit two workgroups if all min(E, n) slots are active, evened out so that no split is empty.
PA_EXPORT int pa_moe_decode_mx_splits(int n, int E, int d, int f) {
  if (n < 1 || E < 1 || d < 128 || f < 128) return 1;
  const int64_t wgs = (int64_t)(d / kMxBand) * (E < n ? E : n), target = 2 * device_cus();
  const int steps = f / 128, most = steps / 2 < 8 ? (steps / 2 < 1 ? 1 : steps / 2) : 8;
  int s = (int)((target + wgs - 1) / wgs);
  s = s < most ? s : most;
  const int per = (steps + s - 1) / s;
  return (steps + per - 1) / per;
}

// Up projection of the MXFP4 expert FFN on a plan of pa_moe_decode_plan: xq [T, d] e4m3fn + xs [T, d / 32] (pa_mx_quant
// of x, mxfp8), w1q [E, 2f, d / 2] + w1s [E, 2f, d / 32] (mxfp4, K-major per expert), b1 [E, 2f] bf16 or null ->
// hq [n, f] e4m3fn + hs [n, f / 32], the mxfp8 quantisation of silu(value) * gate in sorted row order (n = T * topk;
// neither needs clearing). d % 128 == 0, f % 128 == 0.
PA_EXPORT int pa_moe_decode_up_mx(const void* xq, const void* xs, const void* w1q, const void* w1s, const void* b1,
                                  const int* offs, const int* perm, const int* active, const int* n_active, void* hq,
                                  void* hs, int T, int E, int topk, int d, int f, hipStream_t st) {
  if (!moe_decode_mx_shape_ok(T, E, topk, d, f)) return 1;
  MoeDecMxArgs p{};
  p.xq = (const uint8_t*)xq; p.xs = (const uint8_t*)xs; p.w1q = (const uint8_t*)w1q; p.w1s = (const uint8_t*)w1s;
  p.b1 = (const uint16_t*)b1; p.offs = offs; p.perm = perm; p.active = active; p.n_active = n_active;
  p.hq = (uint8_t*)hq; p.hs = (uint8_t*)hs;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk;
  hipLaunchKernelGGL(moe_decode_up_mx_k, dim3(f / kMxBand, E < p.n ? E : p.n), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// Down projection and combine: hq / hs as pa_moe_decode_up_mx leaves them, w2q [E, d, f / 2] + w2s [E, d, f / 32],
// b2 [E, d] bf16 or null, ws = splits * n * d fp32 of workspace (need not be cleared) -> out [T, d] bf16. splits in
// [1, f / 128] with no empty split (as pa_moe_decode_mx_splits returns; 1 is always valid).
PA_EXPORT int pa_moe_decode_down_mx(const void* hq, const void* hs, const void* w2q, const void* w2s, const void* b2,
                                    const float* val, const int* idx, const int* offs, const int* pos,
                                    const int* active, const int* n_active, float* ws, void* out, int T, int E,
                                    int topk, int d, int f, int splits, hipStream_t st) {
  if (!moe_decode_mx_shape_ok(T, E, topk, d, f)) return 1;
  const int steps = f / 128;
  if (splits < 1 || splits > steps) return 2;
  const int per = (steps + splits - 1) / splits;
  if ((steps + per - 1) / per != splits) return 2;
  MoeDecMxArgs p{};
  p.w2q = (const uint8_t*)w2q; p.w2s = (const uint8_t*)w2s; p.offs = offs; p.active = active; p.n_active = n_active;
  p.hq = (uint8_t*)hq; p.hs = (uint8_t*)hs; p.ws = ws;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk; p.steps_per = per;
  hipLaunchKernelGGL(moe_decode_down_mx_k, dim3(d / kMxBand, E < p.n ? E : p.n, splits), dim3(256), 0, st, p);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  MoeDecArgs c{};
  c.b2 = (const uint16_t*)b2; c.val = val; c.idx = idx; c.pos = pos; c.ws = ws; c.out = (uint16_t*)out;
  c.T = T; c.E = E; c.topk = topk; c.d = d; c.f = f; c.n = p.n; c.splits = splits;
  hipLaunchKernelGGL(moe_decode_combine_k, dim3((d / 4 + 255) / 256, T), dim3(256), 0, st, c);
  return (int)hipGetLastError();
}
