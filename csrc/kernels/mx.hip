// OCP Microscaling (MX) linear on the gfx950 block-scaled MFMA: quantiser, tiled GEMM, small-M GEMM.
//
// v_mfma_scale_f32_16x16x128_f8f6f4 multiplies fp4 / fp8 operands that carry one E8M0 scale per 32 k-elements.
// gemm_fp8.hip issues it with both scales pinned to 1.0; here the scales are data. Inference only (forward); every
// scale stays on the device, no launcher reads device memory on the host, none records a memset.
//
// Formats and memory layout (public; paddlepaddle_amd/ops/mx.py holds the same rule in plain torch):
//   * a tensor [R, K] is quantised along K in blocks of 32 (K % 32 == 0);
//   * scales: uint8 [R, K / 32] row-major, an E8M0 exponent byte e with value 2^(e - 127);
//   * mxfp4 elements: e2m1 (0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives; code = sign << 3 | magnitude index),
//     two per byte, uint8 [R, K / 2]; element 2i is the LOW nibble of byte i, element 2i + 1 the high nibble (the
//     order the MFMA consumes a fragment register in);
//   * mxfp8 elements: e4m3fn, uint8 [R, K];
//   * rule (OCP MX v1.0) per block: amax = max|x|; e = clamp(floor(log2 amax) - emax + 127, 0, 254) with emax = 2
//     (e2m1) / 8 (e4m3); elements = x * 2^(127 - e) rounded to nearest even and saturated to +-6 / +-448; amax == 0
//     gives e = 127 and zero elements. An element keeps the sign bit of x (a negative that rounds to 0 is -0).
//     Inputs are finite.
//
// pa_mx_quant: a thread converts 8 consecutive elements (one 16-byte load of 16-bit input, two of fp32), so a 32-block
// lives in 4 adjacent lanes and its amax is two DPP quad swaps; the exponent is the amax's fp32 exponent field minus
// emax (a zero or denormal field clamps to 0), the multiplier 2^(127 - e) is built from bits, e2m1 rounding is the
// add-and-subtract of 2^22 / 2^23 / 2^24 (RNE at steps 0.5 / 1 / 2) and e4m3 the hardware convert after the clamp.
// [R, K] contiguous makes elements and scales flat arrays, so a wave writes 256 (fp4) / 512 (fp8) contiguous
// bytes and its 16 scale bytes leave as four dwords.
//
// pa_gemm_mx: C[M, N] = A[M, K] . B[N, K]^T (+ bias[N]); A mxfp8 or mxfp4, B mxfp4, both K-major; C fp32 / fp16 /
// bf16. Any M, K % 128 == 0, N % 4 == 0 (the lane's 4-column store). The shape of gemm_fp8.hip's generic kernel:
// 256 x 256 tile (128 x 256 with an mxfp8 A), 8 waves as 2 (M) x 4 (N), two 64-KiB LDS stages fed by LDS-DMA in the
// 128-byte-row swizzled image of mfma_tile.h (k_swz on both sides). A stage is 256 k: an fp4 row of 256 k is 128
// bytes, the image of the fp8 kernel byte for byte, read as two MFMA k-steps (chunks 4s + g); an fp8 A needs two such
// images per stage, which is why its tile has half the rows (64 KiB per stage either way, 128 of the 160 KiB).
// K % 256 == 128 ends in a half stage: the staging clamps the k offset inside the row and the second k-step is
// skipped. Operands are swapped (D = B-frag x A-frag) so a lane ends with 4 consecutive columns of one row.
//   Fragments (measured on the hardware; tests/test_mx_gpu.py pins them): of a 128-k step, lane l holds row (l & 15)
// and, with g = l >> 4, for fp4 the 32 elements [32 g, 32 g + 32) (16 contiguous bytes, 4 VGPRs, element 2i in the low
// nibble), for fp8 the bytes [16 g, 16 g + 16) in VGPRs 0-3 and [64 + 16 g, 64 + 16 g + 16) in VGPRs 4-7: the
// instruction runs an fp8 operand as two 64-k halves. The scale it takes from lane l still belongs to the
// k-block [32 g, 32 g + 32) for either format.
//   Scales: lane l presents, in byte 0 of the scale register (op_sel 0), the E8M0 of row (l & 15) and k-block (l >> 4)
// of the 128-k step, once per A fragment and once per B fragment. They come straight from global memory, not through
// LDS: the four k-blocks of a row and k-step are one aligned dword of the public [R, K / 32] layout, a lane loads
// the dword of its row and shifts its byte down, so no re-layout of anyone's scales is needed; the bytes are 1/16
// (fp4) or 1/32 (fp8) of the operand's and are re-read only by the 2 or 4 waves that share the rows (L2 hits); an LDS
// image would add a DMA whose smallest unit (64 lanes x 4 B) does not match a [256][8 B] stage and a second
// swizzle to keep conflict-free. A row's scale registers are refilled for stage t + 1 right after its last MFMA of
// stage t, so the loads fly under the rest of the stage.
//
// pa_gemm_mx_small_m: M <= 64 (decode), bound by the weight bytes, wo_gemm.hip's split of work: a workgroup of 4 waves
// owns 16 NT channels (NT = 1 / 2 / 4 for M <= 16 / 32 / 64) and all rows, waves interleave the 128-k steps, the
// weight fragment (16 contiguous bytes of one row) and its scale byte go from global memory to the MFMA with no LDS
// two steps ahead, the four waves' sums meet in LDS. K may be split over gridDim.y: split s writes its fp32 partial
// into slab s of the workspace [splits][M][N] and mx_finalize_k sums the slabs in a fixed order (no atomics, no
// zeroing, the same bits every run). N % 16 == 0.
#include "common.h"
#include "launch.h"
#include "mfma_tile.h"
#include "mx_block.h"

#include <algorithm>

using namespace pa;

namespace {

// ------------------------------------------------------------------------------------------ quantiser

// e2m1 code of v (already scaled), round to nearest even, saturated at 6
__device__ __forceinline__ uint32_t fp4_code(float v) {
  const uint32_t sign = (__float_as_uint(v) >> 28) & 8u;
  const float a = fminf(fabsf(v), 8.f);
  const float magic = a < 2.f ? 0x1p22f : (a < 4.f ? 0x1p23f : 0x1p24f);  // ulp 0.5 / 1 / 2
  const float r = fminf((a + magic) - magic, 6.f);
  // r >= 1: exponent and top mantissa bit count the codes 2 (1.0) .. 7 (6.0); below: 0.5 -> 1, 0 -> 0
  const uint32_t mag = r >= 1.f ? (__float_as_uint(r) >> 22) - 252u : (r > 0.f ? 1u : 0u);
  return sign | mag;
}

__device__ __forceinline__ float quad_max(float m) {
  m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0xB1, 0xF, 0xF, true)));  // 1,0,3,2
  return fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x4E, 0xF, 0xF, true)));  // 2,3,0,1
}

template <int FMT, typename T>
__global__ __launch_bounds__(256) void mx_quant_k(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                   uint8_t* __restrict__ sc, int64_t nblk) {
  constexpr int EMAX = FMT == kFmtFp4 ? 2 : 8;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;  // 8 elements each, 4 threads per block of 32
  const int64_t blk = tid >> 2;
  const bool ok = blk < nblk;
  float v[8];
  if (ok) {
    load8<T>(x + tid * 8, v);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
  }
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(v[i]));
  m = quad_max(m);
  const int e = mx_block_exp<EMAX>(m);  // finite amax: at most 252
  const float s = mx_block_mult(e);
  if (ok) {
    if constexpr (FMT == kFmtFp4) {
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) w |= fp4_code(v[i] * s) << (4 * i);
      reinterpret_cast<uint32_t*>(q)[tid] = w;
    } else {
      uint32_t w[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float* u = v + 4 * h;
        w[h] = mx_e4m3x2<true>(u[2], u[3], s, mx_e4m3x2<false>(u[0], u[1], s, 0));
      }
      reinterpret_cast<uint2*>(q)[tid] = make_uint2(w[0], w[1]);
    }
  }
  // the wave's 16 scale bytes: lane 16 j collects blocks 4 j .. 4 j + 3 into one dword
  const int lane = threadIdx.x & 63, base = lane & 48;
  const uint32_t pk = (uint32_t)__shfl(e, base, 64) | ((uint32_t)__shfl(e, base + 4, 64) << 8) |
                      ((uint32_t)__shfl(e, base + 8, 64) << 16) | ((uint32_t)__shfl(e, base + 12, 64) << 24);
  if ((lane & 15) == 0 && ok) {
    if (blk + 3 < nblk) {
      *reinterpret_cast<uint32_t*>(sc + blk) = pk;  // blk % 4 == 0
    } else {
      for (int i = 0; i < 4 && blk + i < nblk; ++i) sc[blk + i] = (uint8_t)(pk >> (8 * i));
    }
  }
}

// ------------------------------------------------------------------------------------------ shared by the GEMMs

// one output element in the launcher's out code (0 fp32, 1 fp16, 2 bf16)
__device__ __forceinline__ void store_out(void* c, int64_t i, float v, int out) {
  if (out == 0) reinterpret_cast<float*>(c)[i] = v;
  else if (out == 1) reinterpret_cast<uint16_t*>(c)[i] = (uint16_t)(pack_f16(v, 0.f) & 0xffffu);
  else reinterpret_cast<uint16_t*>(c)[i] = (uint16_t)(pack_bf16(v, 0.f) & 0xffffu);
}

// ------------------------------------------------------------------------------------------ tiled GEMM

struct MxArgs {
  const uint8_t* a;   // [M][K] e4m3fn or [M][K / 2] e2m1 pairs
  const uint8_t* sa;  // [M][K / 32]
  const uint8_t* b;   // [N][K / 2]
  const uint8_t* sb;  // [N][K / 32]
  void* c;            // [M][N]
  const float* bias;  // [N] fp32 or null
  int M, N, K;
  int tiles_m, tiles_n;
};

// stage<R, true> of mfma_tile.h (same image, same k_swz) with the k offset clamped inside the row: the last stage
// of a K % 256 == 128 problem holds one k-step, and its other half must not be read past the row's end
template <int R>
__device__ __forceinline__ void stage_mx(const uint8_t* __restrict__ g, int ld, int r0, int rmax, int k0, int kmax,
                                         char* img, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < R / 64; ++i) {
    const int q = i * 8 + wave;
    const int row = q * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ k_swz(row);
    int gr = r0 + row;
    gr = gr < rmax ? gr : rmax - 1;
    int kb = k0 + lc * 16;
    kb = kb < kmax ? kb : kmax - 16;
    glds16(g + (uint32_t)(gr * ld + kb), img + q * 1024);  // 32-bit offset: the launcher bounds the operand
  }
}

template <int FA, int OUT>
__global__ __launch_bounds__(512, 1) void gemm_mx_kernel(MxArgs p) {
  constexpr int TM = FA == kFmtFp4 ? 256 : 128, TN = 256;
  constexpr int MR = TM / 32, NR = 4;      // wave tile (TM / 2) x 64
  constexpr int kAImg = TM * 128;          // one A image
  constexpr int kABytes = FA == kFmtFp4 ? kAImg : 2 * kAImg;
  constexpr int kStage = kABytes + TN * 128;
  static_assert(kStage == 64 * 1024, "two stages of 64 KiB");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;

  const int nwg = p.tiles_m * p.tiles_n;
  const int pid = xcd_remap((int)blockIdx.x, nwg);
  int tm, tn;
  tile_coords(pid, p.tiles_m, p.tiles_n, &tm, &tn);
  const int m0 = tm * TM, n0 = tn * TN;
  const int lda = FA == kFmtFp4 ? p.K / 2 : p.K, ldb = p.K / 2, lds = p.K / 32;

  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nks = p.K / 128;      // MFMA k-steps
  const int nst = (nks + 1) / 2;  // stages of 256 k
  auto stage_tile = [&](int t, int buf) {
    char* base = smem + buf * kStage;
    if constexpr (FA == kFmtFp4) {
      stage_mx<TM>(p.a, lda, m0, p.M, t * 128, lda, base, wave, lane);
    } else {
      stage_mx<TM>(p.a, lda, m0, p.M, t * 256, lda, base, wave, lane);
      if (2 * t + 1 < nks) stage_mx<TM>(p.a, lda, m0, p.M, t * 256 + 128, lda, base + kAImg, wave, lane);
    }
    stage_mx<TN>(p.b, ldb, n0, p.N, t * 128, ldb, base + kABytes, wave, lane);
  };

  // Scales: a lane holds the dword (4 k-blocks) of each of its fragment rows for the two k-steps of the stage (rows
  // past the edge clamped like the operand rows) and shifts its own byte down in front of the MFMA. The registers of
  // a row are refilled for the next stage right after the row's last MFMA of this one, so the loads fly under the
  // rest of the stage and the barrier, and no second set of registers is needed.
  const int sh = 8 * (lane >> 4);
  const int lo4 = frag_lo(lane, lane >> 4);
  // byte offsets of the rows' scales from the uniform bases (32-bit: the launcher bounds the arrays)
  uint32_t aoff[MR], boff[NR];
#pragma unroll
  for (int i = 0; i < MR; ++i) aoff[i] = (uint32_t)(min(m0 + wm * (TM / 2) + i * 16 + (lane & 15), p.M - 1) * lds);
#pragma unroll
  for (int j = 0; j < NR; ++j) boff[j] = (uint32_t)(min(n0 + wn * 64 + j * 16 + (lane & 15), p.N - 1) * lds);
  uint32_t sa[MR][2], sb[NR][2];
  // the dword of the stage's second k-step; a half stage has none (and the row may end there): it re-reads the first
  auto hi_of = [&](int t) { return 2 * t + 1 < nks ? 4 : 0; };
  auto load_sa = [&](int i, int t) {
    const uint8_t* s = p.sa + 8 * t;
    sa[i][0] = *reinterpret_cast<const uint32_t*>(s + aoff[i]);
    sa[i][1] = *reinterpret_cast<const uint32_t*>(s + hi_of(t) + aoff[i]);
  };
  auto load_sb = [&](int j, int t) {
    const uint8_t* s = p.sb + 8 * t;
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
    const bool more = t + 1 < nst;  // then this stage has both k-steps
    const int tn = more ? t + 1 : t;  // the stage the scale registers are refilled for (the last one: itself, unused)
    if (more) stage_tile(t + 1, cur ^ 1);
    const char* aimg = smem + cur * kStage;
    const char* bimg = aimg + kABytes;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * t + s < nks) {
        i32x8 bf[NR];
        int bs[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          bf[j] = frag4(bimg + (wn * 64 + j * 16) * 128, lo4, s);
          bs[j] = (int)((sb[j][s] >> sh) & 0xffu);
        }
#pragma unroll
        for (int i = 0; i < MR; ++i) {
          const char* ap = aimg + (wm * (TM / 2) + i * 16) * 128;
          const i32x8 af = FA == kFmtFp4 ? frag4(ap, lo4, s) : frag8(ap + s * kAImg, lo4);
          const int as = (int)((sa[i][s] >> sh) & 0xffu);
#pragma unroll
          for (int j = 0; j < NR; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af, acc[i][j], kFmtFp4, FA, 0, bs[j],
                                                                         0, as);
          if (s == 1) load_sa(i, tn);
        }
        if (s == 1) {
#pragma unroll
          for (int j = 0; j < NR; ++j) load_sb(j, tn);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // lane holds C[m = mrow0 + i*16][n = ncol0 + j*16 + 0..3]
  const int mrow0 = m0 + wm * (TM / 2) + (lane & 15);
  const int ncol0 = n0 + wn * 64 + 4 * (lane >> 4);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int n = ncol0 + j * 16;
    if (n >= p.N) continue;  // N % 4 == 0 (launcher)
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bv = *reinterpret_cast<const float4*>(p.bias + n);
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const int m = mrow0 + i * 16;
      if (m >= p.M) continue;
      const float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y, v2 = acc[i][j][2] + bv.z,
                  v3 = acc[i][j][3] + bv.w;
      const int64_t at = (int64_t)m * p.N + n;
      if constexpr (OUT == 0) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.c) + at) = make_float4(v0, v1, v2, v3);
      } else {
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.c) + at) =
            OUT == 1 ? make_uint2(pack_f16(v0, v1), pack_f16(v2, v3)) : make_uint2(pack_bf16(v0, v1), pack_bf16(v2, v3));
      }
    }
  }
}

template <int FA>
int launch_tiled(const MxArgs& g, int out, hipStream_t st) {
  const dim3 grid(g.tiles_m * g.tiles_n), block(512);
  constexpr int lds = 2 * 64 * 1024;
  if (out == 0) return launch_lds<gemm_mx_kernel<FA, 0>>(grid, block, lds, st, g);
  if (out == 1) return launch_lds<gemm_mx_kernel<FA, 1>>(grid, block, lds, st, g);
  return launch_lds<gemm_mx_kernel<FA, 2>>(grid, block, lds, st, g);
}

// ------------------------------------------------------------------------------------------ small-M GEMM

struct MxSmallArgs {
  const uint8_t* a;
  const uint8_t* sa;
  const uint8_t* b;
  const uint8_t* sb;
  void* c;            // [M][N] in the out code (no split)
  const float* bias;  // [N] fp32 or null
  float* ws;          // [split][M][N] fp32 partials (split > 1)
  int M, N, K, steps_per_split, split, out;
};

// MT: 16-row tiles (ceil(M / 16)); NT: 16-channel tiles of the workgroup
template <int FA, int MT, int NT>
__global__ __launch_bounds__(256) void gemm_mx_small_m_k(MxSmallArgs p) {
  constexpr int TILE = MT * 256;  // floats of one 16-channel tile's sums
  constexpr int AK = FA == kFmtFp4 ? 64 : 128;  // A bytes per k-step of a row
  __shared__ float red[4][NT * TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  const int step0 = blockIdx.y * p.steps_per_split;
  const int nst = min(p.steps_per_split, p.K / 128 - step0);
  const int lds = p.K / 32;
  // the lane's weight row (channel) per tile and activation row per row tile, at its k-group; rows past the edge are
  // clamped and their sums dropped
  const uint8_t* wrow[NT];
  const uint8_t* wsc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = min(n0 + j * 16 + col, p.N - 1);
    wrow[j] = p.b + (int64_t)n * (p.K / 2) + (int64_t)step0 * 64 + g * 16;
    wsc[j] = p.sb + (int64_t)n * lds + step0 * 4 + g;
  }
  const uint8_t* arow[MT];
  const uint8_t* asc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = min(t * 16 + col, p.M - 1);
    arow[t] = p.a + (int64_t)m * (AK * (p.K / 128)) + (int64_t)step0 * AK + g * 16;
    asc[t] = p.sa + (int64_t)m * lds + step0 * 4 + g;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // weight stream two of the wave's steps ahead of the MFMAs (the only HBM operand; activations are L2-resident)
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
      raw1[j] = h ? *reinterpret_cast<const uint4*>(wrow[j] + (c + 8) * 64) : make_uint4(0, 0, 0, 0);
      s1[j] = h ? (int)wsc[j][(c + 8) * 4] : 127;
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const uint8_t* ap = arow[t] + (int64_t)c * AK;
      i32x8 af;
      if constexpr (FA == kFmtFp4) af = widen(*reinterpret_cast<const uint4*>(ap));
      else af = join(*reinterpret_cast<const uint4*>(ap), *reinterpret_cast<const uint4*>(ap + 64));
      const int as = (int)asc[t][c * 4];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[t][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf[j], acc[t][j], FA, kFmtFp4, 0, as, 0,
                                                                     bs[j]);
    }
  }
  // D layout: col = lane & 15 (the channel), rows (lane >> 4) * 4 + r of each 16-row tile
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][j * TILE + (t * 16 + g * 4 + r) * 16 + col] = acc[t][j][r];
  __syncthreads();
  for (int e = tid; e < NT * TILE; e += 256) {
    const int j = e / TILE, w = e % TILE;
    const int m = w >> 4, nn = n0 + j * 16 + (w & 15);
    if (m >= p.M || nn >= p.N) continue;
    float v = red[0][e] + red[1][e] + red[2][e] + red[3][e];
    if (p.split > 1) {
      p.ws[((int64_t)blockIdx.y * p.M + m) * p.N + nn] = v;
    } else {
      if (p.bias) v += p.bias[nn];
      store_out(p.c, (int64_t)m * p.N + nn, v, p.out);
    }
  }
}

// C = sum of the split slabs (in slab order) + bias
__global__ __launch_bounds__(256) void mx_finalize_k(const float* __restrict__ ws, const float* __restrict__ bias,
                                                      void* c, int M, int N, int split, int out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, tot = (int64_t)M * N;
  if (i >= tot) return;
  float v = 0.f;
  for (int s = 0; s < split; ++s) v += ws[s * tot + i];
  if (bias) v += bias[i % N];
  store_out(c, i, v, out);
}

// column tiles per workgroup by row count (more rows: more channels per activation fragment)
inline int nt_for(int M) { return M <= 16 ? 1 : (M <= 32 ? 2 : 4); }

template <int FA>
int launch_small(const MxSmallArgs& a, dim3 grid, hipStream_t st) {
  const dim3 block(256);
  switch ((a.M + 15) / 16) {
    case 1: hipLaunchKernelGGL((gemm_mx_small_m_k<FA, 1, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((gemm_mx_small_m_k<FA, 2, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((gemm_mx_small_m_k<FA, 3, 4>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((gemm_mx_small_m_k<FA, 4, 4>), grid, block, 0, st, a); break;
    default: return 1;
  }
  return 0;
}

inline bool fmt_ok(int f) { return f == kFmtFp8 || f == kFmtFp4; }

}  // namespace

// x [R][K] contiguous (in_dtype: 0 fp32, 1 fp16, 2 bf16) -> q (fmt 0: mxfp8 [R][K]; 4: mxfp4 [R][K / 2]) and
// scales [R][K / 32]. K % 32 == 0; x and q 16-byte aligned, scales 4-byte aligned. Returns 1 for a shape it does not take.
PA_EXPORT int pa_mx_quant(const void* x, void* q, void* scales, int64_t R, int64_t K, int in_dtype, int fmt,
                          hipStream_t st) {
  if (R < 0 || K < 0 || K % 32 != 0 || !fmt_ok(fmt)) return 1;
  const int64_t nblk = R * (K / 32);
  if (nblk == 0) return 0;
  const dim3 grid((unsigned)cdiv(nblk * 4, 256)), block(256);
  uint8_t* qp = (uint8_t*)q;
  uint8_t* sp = (uint8_t*)scales;
  PA_DISPATCH_DTYPE(in_dtype, T, {
    if (fmt == kFmtFp4) hipLaunchKernelGGL((mx_quant_k<kFmtFp4, T>), grid, block, 0, st, (const T*)x, qp, sp, nblk);
    else hipLaunchKernelGGL((mx_quant_k<kFmtFp8, T>), grid, block, 0, st, (const T*)x, qp, sp, nblk);
  });
  PA_CHECK_LAUNCH();
  return 0;
}

// C[M][N] = A . B^T (+ bias), all contiguous. fmt_a: 0 mxfp8 / 4 mxfp4; B mxfp4; out: 0 fp32, 1 fp16, 2 bf16; bias
// fp32 [N] or null. Returns 1 for a shape it does not take (K % 128, N % 4, an operand of 2^31 elements or more).
PA_EXPORT int pa_gemm_mx(const void* a, const void* sa, const void* b, const void* sb, void* c, const float* bias,
                         int64_t M, int64_t N, int64_t K, int fmt_a, int out, hipStream_t st) {
  if (K <= 0 || K % 128 != 0 || N % 4 != 0 || !fmt_ok(fmt_a) || out < 0 || out > 2) return 1;
  if (M * K >= (1ll << 31) || N * K >= (1ll << 31)) return 1;  // the kernel's 32-bit operand and scale offsets
  if (M <= 0 || N <= 0) return 0;
  MxArgs g{};
  g.a = (const uint8_t*)a; g.sa = (const uint8_t*)sa; g.b = (const uint8_t*)b; g.sb = (const uint8_t*)sb;
  g.c = c; g.bias = bias;
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.tiles_m = (int)cdiv(M, fmt_a == kFmtFp4 ? 256 : 128);
  g.tiles_n = (int)cdiv(N, 256);
  return fmt_a == kFmtFp4 ? launch_tiled<kFmtFp4>(g, out, st) : launch_tiled<kFmtFp8>(g, out, st);
}

// Splits of K for the small-M kernel: enough workgroups to fill the chip (2 per CU), at least two 128-k steps per
// split, no empty split.
PA_EXPORT int pa_gemm_mx_small_m_splits(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K < 128) return 1;
  const int64_t wgs = cdiv(N, 16 * nt_for((int)M)), steps = K / 128;
  int64_t s = std::min<int64_t>(cdiv(512, wgs), std::max<int64_t>(1, steps / 2));
  s = cdiv(steps, cdiv(steps, s));
  return (int)s;
}

// The same product for M <= 64. N % 16 == 0, K % 128 == 0. splits in [1, K / 128] with no empty split (as
// pa_gemm_mx_small_m_splits returns; 1 is always valid); ws: splits * M * N fp32 when splits > 1 (need not be zeroed).
PA_EXPORT int pa_gemm_mx_small_m(const void* a, const void* sa, const void* b, const void* sb, void* c,
                                 const float* bias, float* ws, int M, int N, int K, int fmt_a, int out, int splits,
                                 hipStream_t st) {
  if (M <= 0 || M > 64 || N <= 0 || N % 16 != 0 || K <= 0 || K % 128 != 0) return 1;
  if (!fmt_ok(fmt_a) || out < 0 || out > 2) return 2;
  const int steps = K / 128;
  if (splits < 1 || splits > steps) return 5;
  const int per = (steps + splits - 1) / splits;
  if ((steps + per - 1) / per != splits) return 5;
  if (splits > 1 && ws == nullptr) return 6;
  MxSmallArgs g{};
  g.a = (const uint8_t*)a; g.sa = (const uint8_t*)sa; g.b = (const uint8_t*)b; g.sb = (const uint8_t*)sb;
  g.c = c; g.bias = bias; g.ws = ws;
  g.M = M; g.N = N; g.K = K; g.steps_per_split = per; g.split = splits; g.out = out;
  const dim3 grid((unsigned)cdiv(N, 16 * nt_for(M)), (unsigned)splits);
  const int rc = fmt_a == kFmtFp4 ? launch_small<kFmtFp4>(g, grid, st) : launch_small<kFmtFp8>(g, grid, st);
  if (rc) return rc;
  if (splits > 1) {
    const int64_t tot = (int64_t)M * N;
    hipLaunchKernelGGL(mx_finalize_k, dim3((unsigned)cdiv(tot, 256)), dim3(256), 0, st, ws, bias, c, M, N, splits, out);
  }
  PA_CHECK_LAUNCH();
  return 0;
}
