// MoE decode over weight-only int8 / int4 expert weights: the two projections of fused_moe(quant_method=
// "weight_only_int8" | "weight_only_int4") for at most 64 tokens, between moe_decode.hip's plan (pa_moe_decode_plan)
// and the shared combine (moe_combine.h). Four launches, no host read, static shapes: the call captures into a hipGraph.
// Reference behaviour: python/paddle/incubate/nn/functional/fused_moe.py:20 (quant_method), weight layout of
// python/paddle/nn/quant/quantized_linear.py:56 per expert with per-channel scales: w1_q [E, 2f, d] int8 or [E, f, d]
// int4 pairs (channels 2j / 2j + 1 of the 2f in the low / high nibble, stored + 8), w1_s [E, 2f] fp32; w2_q [E, d, f]
// int8 or [E, d / 2, f] pairs, w2_s [E, d] fp32. All 16 nibble codes decode (code 0 is -8).
//
// Decode MoE is bound by the routed experts' weight bytes, so both kernels stream the codes once, from global memory
// straight into registers, the way wo_gemm.hip's wo_gemm_k does for one dense weight:
//   * a workgroup = 4 waves owns four 16-channel MFMA tiles of one active expert (grid: bands x slots (x K splits),
//     a slot past *n_active exits at once) and all of the expert's rows; its waves take interleaved 64-deep K chunks
//     (adjacent waves read adjacent bytes). Per chunk a lane loads 16 bytes along K of one channel row, two of its
//     wave's chunks ahead of the MFMAs, turns the integers into exact bf16 and runs two v_mfma_f32_16x16x32_bf16 per
//     row fragment and tile; A and B use the same permuted k order (lane group q holds k = 16 q .. 16 q + 15);
//   * int4: a lane's 16 bytes are a pair-row, loaded once: the low nibbles are the fragment of channel 2j, the high
//     nibbles that of channel 2j + 1, so a load feeds two tiles with an even / odd channel map and the four tiles
//     need two loads where int8 needs four;
//   * the A rows are not a gathered copy: the up projection reads x[perm[row] / topk] and the down projection h[row]
//     through the lane's own pointer (L2 hits). Rows past the expert's count are clamped reads that are never stored;
//   * the loop over 16-row fragments runs to ceil(rows of this expert / 16), uniform in the workgroup, not to
//     ceil(T / 16): at 64 tokens over many experts most experts hold one or two rows. Accumulators stay statically
//     indexed (unrolled over 4, skipped on the uniform predicate);
//   * the four waves' partial sums meet in LDS and are added in wave order; the per-channel scale multiplies the
//     finished sum.
// moe_decode_up_wo_k: tiles 0, 1 are 32 value channels [n0, n0 + 32), tiles 2, 3 the gate channels f + n, so scale,
// bias and silu(value) * gate run on the sums and h [n, f] is written once, in bf16.
// moe_decode_down_wo_k: 64 channels of d, K = f split over gridDim.z in whole 64-chunks into fp32 slabs
// [split][n][d]; every row of every slab is written (a sorted row belongs to exactly one expert), so there is no
// memset and no atomic and the result is bit-identical from run to run. The scale is applied before the slab write;
// b2, val and the sum over a token's experts stay in moe_decode_combine_k.
//   Deviations from the plain sketch: the cross-wave reduction runs one row fragment at a time through a 16-KiB
// buffer (as the MXFP4 kernels of moe_decode.hip do) instead of holding all four fragments; the down projection's
// band is 64 channels, not 32, so that an activation fragment (32 bytes a lane) feeds four weight tiles.
#include "launch.h"
#include "moe_combine.h"

namespace pa {
namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kWoMaxT = 64, kWoMaxE = 256, kWoMaxTopk = 8, kWoTiles = 4;

struct MoeDecWoArgs {
  const uint16_t* x;         // [T, d] bf16
  const uint8_t *w1q, *w2q;  // codes, K-major per expert
  const float *w1s, *w2s;    // [E, 2f], [E, d]
  const uint16_t* b1;        // [E, 2f] bf16 or null
  const int *offs, *perm, *active, *n_active;
  uint16_t* h;               // [n, f] bf16, sorted row order
  float* ws;                 // [splits, n, d] fp32
  int T, E, topk, d, f, n, ch_per;
};

// the expert of this slot and its sorted rows [r0, r0 + cnt); false for a slot with nothing to do or a plan that
// does not fit the buffers
__device__ __forceinline__ bool moe_wo_slot(const MoeDecWoArgs& p, int slot, int& e, int& r0, int& cnt) {
  if (slot >= *p.n_active) return false;
  e = p.active[slot];
  if ((unsigned)e >= (unsigned)p.E) return false;
  r0 = p.offs[e];
  if (r0 < 0 || r0 >= p.n) return false;
  cnt = min(min(p.offs[e + 1] - r0, kWoMaxT), p.n - r0);
  return cnt > 0;
}

// 16-byte loads a lane makes per chunk for the four tiles
template <int BITS>
constexpr int wo_loads() { return BITS == 8 ? 4 : 2; }
// chunks of its own a wave keeps in flight ahead of the MFMAs; 3 (int8) and 4 (int4) measured no faster than 2
constexpr int kWoDepth = 2;

// The lane's weight rows (at k-group q of chunk 0) for two 32-channel groups starting at channels c0 and c1 of the
// expert's matrix ``w`` (rows of ld bytes). int8: load 2 g + h is channel cg + 16 h + col; int4: load g is pair-row
// cg / 2 + col, channels cg + 2 col + {0, 1}.
template <int BITS>
__device__ __forceinline__ void wo_rows(const uint8_t* w, int64_t ld, int c0, int c1, int col, int q,
                                        const uint8_t* (&wrow)[wo_loads<BITS>()]) {
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int cg = g ? c1 : c0;
    if constexpr (BITS == 8) {
      wrow[2 * g] = w + (int64_t)(cg + col) * ld + q * 16;
      wrow[2 * g + 1] = w + (int64_t)(cg + 16 + col) * ld + q * 16;
    } else {
      wrow[g] = w + (int64_t)(cg / 2 + col) * ld + q * 16;
    }
  }
}

// where channel c (0 .. 31) of group g sits in a fragment's [4 tiles][16 rows][16 columns] sums, row 0
template <int BITS>
__device__ __forceinline__ int wo_red_at(int g, int c) {
  return BITS == 8 ? (2 * g + (c >> 4)) * 256 + (c & 15) : (2 * g + (c & 1)) * 256 + (c >> 1);
}

// two small integers as a bf16 pair: exact, so the high halves of the floats are the bf16 bits
__device__ __forceinline__ uint32_t wo_bf16x2(int a, int b) {
  return __builtin_amdgcn_perm(__float_as_uint((float)b), __float_as_uint((float)a), 0x07060302u);
}

// 16 codes along K -> the fragments of the two MFMAs (k 0 .. 7 and 8 .. 15 of the lane's group). HI: the high nibbles.
template <int BITS, bool HI>
__device__ __forceinline__ void wo_dequant(const uint4& raw, bf16x8& lo, bf16x8& hi) {
  const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 16; i += 2) {
    int v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t byte = wd[(i + u) >> 2] >> (8 * ((i + u) & 3));
      if constexpr (BITS == 8) v[u] = (int)(int8_t)(byte & 0xffu);
      else v[u] = (int)((HI ? byte >> 4 : byte) & 0xfu) - 8;
    }
    o[i >> 1] = wo_bf16x2(v[0], v[1]);
  }
  lo = __builtin_bit_cast(bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
  hi = __builtin_bit_cast(bf16x8, make_uint4(o[4], o[5], o[6], o[7]));
}

// The K loop of both projections: this wave's 64-chunks wave, wave + 4, ... of nch. wrow: the lane's weight rows;
// arow: the lane's activation row (row lane & 15 of each fragment) at k-group q of chunk 0. The weight stream, the only
// operand that comes from HBM, runs two of the wave's chunks ahead; fragments past nfrag (wave-uniform) are skipped.
template <int BITS>
__device__ __forceinline__ void moe_wo_stream(const uint8_t* const (&wrow)[wo_loads<BITS>()],
                                              const uint16_t* const (&arow)[4], int nfrag, int nch, int wave,
                                              f32x4 (&acc)[4][kWoTiles]) {
  constexpr int NL = wo_loads<BITS>(), D = kWoDepth;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < kWoTiles; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 raw[D][NL];
#pragma unroll
  for (int s = 0; s < D; ++s)
#pragma unroll
    for (int l = 0; l < NL; ++l)
      raw[s][l] = wave + 4 * s < nch ? *reinterpret_cast<const uint4*>(wrow[l] + (wave + 4 * s) * 64)
                                     : make_uint4(0, 0, 0, 0);
  for (int c = wave; c < nch; c += 4) {
    bf16x8 blo[kWoTiles], bhi[kWoTiles];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if constexpr (BITS == 8) {
        wo_dequant<8, false>(raw[0][l], blo[l], bhi[l]);
      } else {
        wo_dequant<4, false>(raw[0][l], blo[2 * l], bhi[2 * l]);
        wo_dequant<4, true>(raw[0][l], blo[2 * l + 1], bhi[2 * l + 1]);
      }
#pragma unroll
      for (int s = 0; s + 1 < D; ++s) raw[s][l] = raw[s + 1][l];
      raw[D - 1][l] = c + 4 * D < nch ? *reinterpret_cast<const uint4*>(wrow[l] + (int64_t)(c + 4 * D) * 64)
                                      : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= nfrag) continue;
      const uint16_t* ap = arow[t] + (int64_t)c * 64;
      const bf16x8 alo = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ap));
      const bf16x8 ahi = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ap + 8));
#pragma unroll
      for (int j = 0; j < kWoTiles; ++j) {
        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, blo[j], acc[t][j], 0, 0, 0);
        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bhi[j], acc[t][j], 0, 0, 0);
      }
    }
  }
}

// one fragment's partial sums of this wave into red[wave]: tile j at j * 256, [16 rows][16 channels]. The MFMA leaves
// channel lane & 15 and rows 4 (lane >> 4) + r in the lane.
__device__ __forceinline__ void moe_wo_put(float (&red)[4][kWoTiles * 256], const f32x4 (&a)[kWoTiles], int wave,
                                           int lane) {
#pragma unroll
  for (int j = 0; j < kWoTiles; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][j * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)] = a[j][r];
}
__device__ __forceinline__ float moe_wo_sum(const float (&red)[4][kWoTiles * 256], int i) {
  return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// Up projection + SwiGLU. grid (f / 32, slots).
template <int BITS>
__global__ __launch_bounds__(256) void moe_decode_up_wo_k(MoeDecWoArgs p) {
  __shared__ float red[4][kWoTiles * 256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, q = lane >> 4;
  int e, r0, cnt;
  if (!moe_wo_slot(p, blockIdx.y, e, r0, cnt)) return;
  const int n0 = blockIdx.x * 32, nfrag = (cnt + 15) >> 4;
  const uint8_t* wrow[wo_loads<BITS>()];
  wo_rows<BITS>(p.w1q + (int64_t)e * (BITS == 8 ? 2 : 1) * p.f * p.d, p.d, n0, p.f + n0, col, q, wrow);
  // row gather: the token of the lane's row of each fragment
  const uint16_t* arow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int m = min(t * 16 + col, cnt - 1);
    const int tok = min(max(p.perm[r0 + m] / p.topk, 0), p.T - 1);
    arow[t] = p.x + (int64_t)tok * p.d + q * 16;
  }
  f32x4 acc[4][kWoTiles];
  moe_wo_stream<BITS>(wrow, arow, nfrag, p.d / 64, wave, acc);

  // epilogue, a fragment at a time: thread -> row tid >> 4 of the fragment, channels 2 (tid & 15) + {0, 1} of the band
  const int ml = tid >> 4, c2 = (tid & 15) * 2;
  const int64_t cv = (int64_t)e * 2 * p.f + n0 + c2;
  const float sa[2] = {p.w1s[cv], p.w1s[cv + 1]}, sg[2] = {p.w1s[cv + p.f], p.w1s[cv + p.f + 1]};
  float ba[2] = {0.f, 0.f}, bg[2] = {0.f, 0.f};
  if (p.b1) {
    const uint32_t va = *reinterpret_cast<const uint32_t*>(p.b1 + cv);
    const uint32_t vg = *reinterpret_cast<const uint32_t*>(p.b1 + cv + p.f);
    ba[0] = lo_bf16(va); ba[1] = hi_bf16(va); bg[0] = lo_bf16(vg); bg[1] = hi_bf16(vg);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nfrag) continue;
    moe_wo_put(red, acc[t], wave, lane);
    __syncthreads();
    float h[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float a = moe_wo_sum(red, wo_red_at<BITS>(0, c2 + u) + ml * 16) * sa[u] + ba[u];
      const float g = moe_wo_sum(red, wo_red_at<BITS>(1, c2 + u) + ml * 16) * sg[u] + bg[u];
      h[u] = silu(a) * g;
    }
    const int m = t * 16 + ml;
    if (m < cnt) *reinterpret_cast<uint32_t*>(p.h + (int64_t)(r0 + m) * p.f + n0 + c2) = pack_bf16(h[0], h[1]);
    __syncthreads();
  }
}

// Down projection: rows of h x 64 channels of w2_q[e] over the chunks of split blockIdx.z -> fp32 slab.
// grid (d / 64, slots, splits).
template <int BITS>
__global__ __launch_bounds__(256) void moe_decode_down_wo_k(MoeDecWoArgs p) {
  __shared__ float red[4][kWoTiles * 256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, q = lane >> 4;
  int e, r0, cnt;
  if (!moe_wo_slot(p, blockIdx.y, e, r0, cnt)) return;
  const int n0 = blockIdx.x * 64, nfrag = (cnt + 15) >> 4;
  const int ch0 = blockIdx.z * p.ch_per, nch = min(p.ch_per, p.f / 64 - ch0);
  const uint8_t* wrow[wo_loads<BITS>()];
  wo_rows<BITS>(p.w2q + (int64_t)e * (p.d / (BITS == 8 ? 1 : 2)) * p.f + (int64_t)ch0 * 64, p.f, n0, n0 + 32, col, q,
                wrow);
  const uint16_t* arow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    arow[t] = p.h + (int64_t)(r0 + min(t * 16 + col, cnt - 1)) * p.f + (int64_t)ch0 * 64 + q * 16;
  f32x4 acc[4][kWoTiles];
  moe_wo_stream<BITS>(wrow, arow, nfrag, nch, wave, acc);

  // thread -> channel tid & 63 of the band, rows (tid >> 6) + 4 u of the fragment: a row's band is 256 bytes
  const int c = tid & 63;
  const float s = p.w2s[(int64_t)e * p.d + n0 + c];
  const int at = wo_red_at<BITS>(c >> 5, c & 31);
  float* slab = p.ws + ((int64_t)blockIdx.z * p.n + r0) * p.d + n0 + c;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nfrag) continue;
    moe_wo_put(red, acc[t], wave, lane);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ml = (tid >> 6) + 4 * u, m = t * 16 + ml;
      const float v = moe_wo_sum(red, at + ml * 16) * s;
      if (m < cnt) slab[(int64_t)m * p.d] = v;
    }
    __syncthreads();
  }
}

bool moe_decode_wo_shape_ok(int T, int E, int topk, int d, int f, int bits) {
  return T >= 1 && T <= kWoMaxT && E >= 1 && E <= kWoMaxE && topk >= 1 && topk <= kWoMaxTopk && topk <= E &&
         d >= 64 && f >= 64 && d % 64 == 0 && f % 64 == 0 && (bits == 8 || bits == 4);
}

// chunks of a split when f / 64 chunks are split ``splits`` ways; 0 when a split would be empty
int moe_decode_wo_per(int f, int splits) {
  const int chunks = f / 64;
  if (splits < 1 || splits > chunks) return 0;
  const int per = (chunks + splits - 1) / splits;
  return (chunks + per - 1) / per == splits ? per : 0;
}

}  // namespace
}  // namespace pa

using namespace pa;

// K splits of the weight-only down projection by default: the fewest (at most 8, each at least two chunks a wave in
// int8 and four in int4: the same 512 bytes of a channel row) that give every compute unit two workgroups if all
// min(E, n) slots are active, evened out so that no split is empty.
PA_EXPORT int pa_moe_decode_wo_splits(int n, int E, int d, int f, int bits) {
  if (n < 1 || E < 1 || d < 64 || f < 64) return 1;
  const int64_t wgs = (int64_t)(d / 64) * (E < n ? E : n), target = 2 * device_cus();
  const int chunks = f / 64, least = bits == 4 ? 16 : 8;
  const int most = chunks / least < 1 ? 1 : (chunks / least < 8 ? chunks / least : 8);
  int s = (int)((target + wgs - 1) / wgs);
  s = s < most ? s : most;
  const int per = (chunks + s - 1) / s;
  return (chunks + per - 1) / per;
}

// Up projection of the weight-only expert FFN on a plan of pa_moe_decode_plan: x [T, d] bf16, w1q [E, 2f, d] int8
// (bits 8) or [E, f, d] int4 pairs (bits 4), w1s [E, 2f] fp32, b1 [E, 2f] bf16 or null -> h [n, f] bf16 =
// silu(value) * gate in sorted row order (n = T * topk; needs no clearing). d % 64 == 0, f % 64 == 0.
PA_EXPORT int pa_moe_decode_up_wo(const void* x, const void* w1q, const float* w1s, const void* b1, const int* offs,
                                  const int* perm, const int* active, const int* n_active, void* h, int T, int E,
                                  int topk, int d, int f, int bits, hipStream_t st) {
  if (!moe_decode_wo_shape_ok(T, E, topk, d, f, bits)) return 1;
  MoeDecWoArgs p{};
  p.x = (const uint16_t*)x; p.w1q = (const uint8_t*)w1q; p.w1s = w1s; p.b1 = (const uint16_t*)b1;
  p.offs = offs; p.perm = perm; p.active = active; p.n_active = n_active; p.h = (uint16_t*)h;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk;
  const dim3 grid(f / 32, E < p.n ? E : p.n);
  if (bits == 8) hipLaunchKernelGGL(moe_decode_up_wo_k<8>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(moe_decode_up_wo_k<4>, grid, dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// Down projection and combine: h as pa_moe_decode_up_wo leaves it, w2q [E, d, f] int8 or [E, d / 2, f] int4 pairs,
// w2s [E, d] fp32, b2 [E, d] bf16 or null, ws = splits * n * d fp32 of workspace (need not be cleared) -> out [T, d]
// bf16. splits in [1, f / 64] with no empty split (as pa_moe_decode_wo_splits returns; 1 is always valid).
PA_EXPORT int pa_moe_decode_down_wo(const void* h, const void* w2q, const float* w2s, const void* b2, const float* val,
                                    const int* idx, const int* offs, const int* pos, const int* active,
                                    const int* n_active, float* ws, void* out, int T, int E, int topk, int d, int f,
                                    int bits, int splits, hipStream_t st) {
  if (!moe_decode_wo_shape_ok(T, E, topk, d, f, bits)) return 1;
  const int per = moe_decode_wo_per(f, splits);
  if (per == 0) return 2;
  MoeDecWoArgs p{};
  p.w2q = (const uint8_t*)w2q; p.w2s = w2s; p.offs = offs; p.active = active; p.n_active = n_active;
  p.h = (uint16_t*)h; p.ws = ws;
  p.T = T; p.E = E; p.topk = topk; p.d = d; p.f = f; p.n = T * topk; p.ch_per = per;
  const dim3 grid(d / 64, E < p.n ? E : p.n, splits);
  if (bits == 8) hipLaunchKernelGGL(moe_decode_down_wo_k<8>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(moe_decode_down_wo_k<4>, grid, dim3(256), 0, st, p);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  MoeDecArgs c{};
  c.b2 = (const uint16_t*)b2; c.val = val; c.idx = idx; c.pos = pos; c.ws = ws; c.out = (uint16_t*)out;
  c.T = T; c.E = E; c.topk = topk; c.d = d; c.f = f; c.n = p.n; c.splits = splits;
  hipLaunchKernelGGL(moe_decode_combine_k, dim3((d / 4 + 255) / 256, T), dim3(256), 0, st, c);
  return (int)hipGetLastError();
}
