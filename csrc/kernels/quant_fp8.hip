// Per-tensor scaled fp8 quantisation for gfx950: the operand side of the fp8 GEMM (gemm_fp8.hip) in a training step.
// Reference recipe: per-tensor amax scaling with an amax history ("FP8 Formats for Deep Learning", Micikevicius et
// al. 2022); encodings are OCP e4m3fn / e5m2 (gfx950's native ones), as in gemm_fp8.hip.
//
//   pa_fp8_amax          |x|max of a contiguous tensor as per-workgroup partials (no atomics)
//   pa_fp8_scale_update  partials (+ amax history) -> scale = (fmax / amax) * 2^-margin and 1 / scale, on the device
//   pa_fp8_quant         q = sat(x * *scale) as fp8, optionally q^T from the same read and the |x|max partials
//
// The absolute maximum is taken on the fp32 bit pattern (bits & 0x7fffffff, compared unsigned): for finite values
// that is the ordinary maximum, and an inf or NaN anywhere comes out as a non-finite maximum (fmaxf would drop a NaN).
// Partials: kParts fp32 slots, slot b written by workgroup b of a persistent grid, the slots past the grid by
// workgroup 0 as zeros, so every launch leaves the whole buffer defined.
#include "multi_tensor.h"

using namespace pa;

namespace {

constexpr int kParts = 1024;  // slots of a partials buffer = cap of the persistent grids
constexpr int kT = 128;       // tile edge of the transposing kernel

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// maximum over the 256 threads of the workgroup; every thread gets it. red: 4 words of LDS
__device__ __forceinline__ uint32_t block_umax(uint32_t m, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = umax(m, (uint32_t)__shfl_xor((int)m, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return umax(umax(red[0], red[1]), umax(red[2], red[3]));
}

// workgroup b's partial into slot b; workgroup 0 zeroes the slots no workgroup owns
__device__ __forceinline__ void write_part(uint32_t m, uint32_t* red, float* parts) {
  m = block_umax(m, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = __uint_as_float(m);
  if (blockIdx.x == 0)
    for (int i = gridDim.x + threadIdx.x; i < kParts; i += 256) parts[i] = 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void fp8_amax_k(const T* __restrict__ x, int64_t n, float* __restrict__ parts) {
  constexpr int P = V16<T>::kPer;
  constexpr int kUnroll = 4;  // 16-byte requests in flight per lane
  __shared__ uint32_t red[4];
  uint32_t m = 0;
  int64_t nv = 0;
  if ((((uintptr_t)x) & 15) == 0) {
    nv = (n / P) * P;
    const int64_t stride = (int64_t)gridDim.x * 256 * P;
    int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * P;
    for (; i + (kUnroll - 1) * stride < nv; i += kUnroll * stride) {
      float v[kUnroll][P];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) V16<T>::ld(x + i + u * stride, v[u]);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
#pragma unroll
        for (int j = 0; j < P; ++j) m = umax(m, abs_bits(v[u][j]));
    }
    for (; i < nv; i += stride) {
      float v[P];
      V16<T>::ld(x + i, v);
#pragma unroll
      for (int j = 0; j < P; ++j) m = umax(m, abs_bits(v[j]));
    }
  }
  // scalar tail (the whole tensor when x is not 16-byte aligned)
  for (int64_t i = nv + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m = umax(m, abs_bits(to_f(x[i])));
  write_part(m, red, parts);
}

// One workgroup. mode 0: a = the fresh amax; mode 1: the history moves up by one slot, takes the fresh amax at
// slot 0, and a = max(history). A non-finite fresh amax changes nothing; a == 0 leaves the scales as they are.
__global__ __launch_bounds__(256) void fp8_scale_update_k(const float* __restrict__ parts, int n_parts,
                                                          float* __restrict__ hist, int hist_len,
                                                          float* __restrict__ scale, float* __restrict__ scale_inv,
                                                          float fmax, int margin, int mode) {
  __shared__ uint32_t red[4];
  const int t = threadIdx.x;
  uint32_t m = 0;
  for (int i = t; i < n_parts; i += 256) m = umax(m, abs_bits(parts[i]));
  m = block_umax(m, red);
  if (!finite_bits(m)) return;
  uint32_t a = m;
  if (mode == 1) {
    constexpr int kPer = 4;  // hist_len <= 1024 (launcher)
    uint32_t old[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = t + k * 256;
      old[k] = i == 0 ? m : (i < hist_len ? __float_as_uint(hist[i - 1]) : 0u);
    }
    __syncthreads();  // every old slot is in a register before any slot is overwritten
    uint32_t hm = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = t + k * 256;
      if (i < hist_len) {
        hist[i] = __uint_as_float(old[k]);
        hm = umax(hm, old[k] & 0x7fffffffu);
      }
    }
    a = block_umax(hm, red);
  }
  if (t == 0 && finite_bits(a) && a != 0) {
    const float sc = (fmax / __uint_as_float(a)) * __uint_as_float((uint32_t)(127 - margin) << 23);
    *scale = sc;
    *scale_inv = 1.f / sc;
  }
}

// ---- conversion: v * s clamped to +-fmax (a NaN stays a NaN: both comparisons are false), then the hardware
// round-to-nearest-even convert, which keeps fp8 denormals. FMT 0 = e4m3fn (fmax 448), 1 = e5m2 (fmax 57344).
template <int FMT> __device__ __forceinline__ float sat(float v) {
  constexpr float kMax = FMT == 0 ? 448.f : 57344.f;
  v = v > kMax ? kMax : v;
  return v < -kMax ? -kMax : v;
}
template <int FMT> __device__ __forceinline__ uint32_t cvt_pk(float a, float b, uint32_t old, bool hi) {
  if (FMT == 0) return hi ? (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, true)
                          : (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, false);
  return hi ? (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, (int)old, true)
            : (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, (int)old, false);
}
template <int FMT> __device__ __forceinline__ uint32_t cvt4(const float* v, float s) {
  uint32_t w = cvt_pk<FMT>(sat<FMT>(v[0] * s), sat<FMT>(v[1] * s), 0u, false);
  return cvt_pk<FMT>(sat<FMT>(v[2] * s), sat<FMT>(v[3] * s), w, true);
}

// ---- LDS image of a 128 x 128 fp8 tile, 128-byte rows, addressed in 8-byte chunks (16 per row).
// Written row-wise (ds_write_b64: 16 consecutive lanes = the 16 chunks of one row = 32 different banks under any
// permutation of rows or chunks) and read as 8 x 8 blocks: lane (rb, cb) of the second phase reads chunk cb of rows
// 8 rb .. 8 rb + 7, so 16 consecutive lanes read one chunk column of 16 rows that are 8 apart: with plain rows, the
// same two banks 16 times. The chunk is therefore XORed with rb = (r >> 3) & 15: those 16 lanes then read the 16
// different chunks of a 128-byte row (conflict-free under the 32-bank rule of ds_read2_b64, which the compiler
// pairs these reads into). For an unpaired ds_read_b64 (64 banks, 32-lane groups = rb 0..15 x two neighbouring cb)
// row bits 0 and 3 are exchanged as well: the 128-byte half of the bank row is then rb & 1, and the 8 rb of one
// parity x 2 cb take the 16 chunks of their half.
__device__ __forceinline__ int tile_off(int r, int c8) {
  const int pr = (r & ~9) | ((r & 1) << 3) | ((r >> 3) & 1);
  return pr * kT + ((c8 ^ ((r >> 3) & 15)) << 3);
}

// 4 x 4 byte transpose: w[i] = row i -> t[j] = column j (byte i of t[j] = byte j of w[i])
__device__ __forceinline__ void tr4(const uint32_t* w, uint32_t* t) {
  const uint32_t a0 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u);  // rows 0, 1 interleaved: bytes 0, 1
  const uint32_t a1 = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u);  //                         bytes 2, 3
  const uint32_t b0 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);  // rows 2, 3
  const uint32_t b1 = __builtin_amdgcn_perm(w[3], w[2], 0x07030602u);
  t[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u);
  t[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
  t[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u);
  t[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
}

// Vector path (C % 8 == 0, x 16-byte and q 8-byte aligned). A workgroup takes 128 x 128 tiles. Phase 1: thread
// (wr, wc) loads 8 elements (16 bytes; fp32: 2 x 16) of rows 16 k + wr, k = 0..7 — 16 lanes cover 128 columns of a
// row — converts them, stores 8 bytes of q and the same 8 bytes into the LDS image. Phase 2 (qT only): thread
// (rb, cb) transposes one 8 x 8 block in registers and stores 8 bytes along R for each of its 8 columns — 16 lanes
// cover 128 rows of one qT row. qt_vec: R % 8 == 0 and qT 8-byte aligned; otherwise those stores go byte by byte.
template <typename T, int FMT>
__global__ __launch_bounds__(256) void fp8_quant_tile_k(const T* __restrict__ x, int64_t R, int64_t C,
                                                        const float* __restrict__ scale_p, uint8_t* __restrict__ q,
                                                        uint8_t* __restrict__ qT, float* __restrict__ parts,
                                                        int64_t tiles, int tiles_c, int qt_vec) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kT * kT];
  __shared__ uint32_t red[4];
  const float s = *scale_p;
  const int t = threadIdx.x;
  const int wr = t >> 4, wc = t & 15;
  const int rb = t & 15, cb = t >> 4;
  uint32_t m = 0;
  for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const int64_t r0 = (tl / tiles_c) * kT, c0 = (tl % tiles_c) * kT;
    const int64_t c = c0 + wc * 8;
    float v[8][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t r = r0 + k * 16 + wr;
      if (r < R && c < C) {
        load8<T>(x + r * C + c, v[k]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t r = r0 + k * 16 + wr;
#pragma unroll
      for (int j = 0; j < 8; ++j) m = umax(m, abs_bits(v[k][j]));
      const uint2 w = make_uint2(cvt4<FMT>(v[k], s), cvt4<FMT>(v[k] + 4, s));
      if (r < R && c < C) *reinterpret_cast<uint2*>(q + r * C + c) = w;
      if (qT) *reinterpret_cast<uint2*>(tile + tile_off(k * 16 + wr, wc)) = w;
    }
    if (!qT) continue;  // uniform
    __syncthreads();
    uint32_t lo[8], hi[8], o[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint2 w = *reinterpret_cast<const uint2*>(tile + tile_off(rb * 8 + i, cb));
      lo[i] = w.x; hi[i] = w.y;
    }
    // o[2 j], o[2 j + 1]: column j of the block, rows 0..3 and 4..7
    uint32_t tt[4];
    tr4(lo, tt);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[2 * j] = tt[j];
    tr4(lo + 4, tt);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[2 * j + 1] = tt[j];
    tr4(hi, tt);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[8 + 2 * j] = tt[j];
    tr4(hi + 4, tt);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[8 + 2 * j + 1] = tt[j];
    const int64_t rr = r0 + rb * 8;
    if (rr < R) {
      const bool whole = qt_vec && rr + 8 <= R;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t cc = c0 + cb * 8 + j;
        if (cc >= C) break;
        uint8_t* dst = qT + cc * R + rr;
        if (whole) {
          *reinterpret_cast<uint2*>(dst) = make_uint2(o[2 * j], o[2 * j + 1]);
        } else {
          for (int b = 0; b < 8 && rr + b < R; ++b)
            dst[b] = (uint8_t)((b < 4 ? o[2 * j] >> (8 * b) : o[2 * j + 1] >> (8 * (b - 4))) & 0xff);
        }
      }
    }
    __syncthreads();  // the image is free for the next tile
  }
  if (parts) write_part(m, red, parts);
}

// Scalar path: any C, any alignment; one element per thread and trip.
template <typename T, int FMT>
__global__ __launch_bounds__(256) void fp8_quant_scalar_k(const T* __restrict__ x, int64_t R, int64_t C,
                                                          const float* __restrict__ scale_p,
                                                          uint8_t* __restrict__ q, uint8_t* __restrict__ qT,
                                                          float* __restrict__ parts) {
  __shared__ uint32_t red[4];
  const float s = *scale_p;
  const int64_t n = R * C;
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = to_f(x[i]);
    m = umax(m, abs_bits(v));
    const uint8_t b = (uint8_t)(cvt_pk<FMT>(sat<FMT>(v * s), 0.f, 0u, false) & 0xff);
    q[i] = b;
    if (qT) qT[(i % C) * R + i / C] = b;
  }
  if (parts) write_part(m, red, parts);
}

template <typename T, int FMT>
int quant_launch(const void* x, int64_t R, int64_t C, const float* scale, uint8_t* q, uint8_t* qT, float* parts,
                 hipStream_t st) {
  const bool vec = C % 8 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)q) & 7) == 0;
  if (vec) {
    const int64_t tiles_c = cdiv(C, kT), tiles = cdiv(R, kT) * tiles_c;
    // every workgroup of the persistent grid gets the same number of tiles, give or take one
    const int64_t trips = cdiv(tiles, kParts), grid = cdiv(tiles, trips);
    const int qt_vec = R % 8 == 0 && (((uintptr_t)qT) & 7) == 0;
    hipLaunchKernelGGL((fp8_quant_tile_k<T, FMT>), dim3((unsigned)grid), dim3(256), 0, st, (const T*)x, R, C, scale, q,
                       qT, parts, tiles, (int)tiles_c, qt_vec);
  } else {
    const int64_t wgs = cdiv(R * C, 256);
    hipLaunchKernelGGL((fp8_quant_scalar_k<T, FMT>), dim3((unsigned)(wgs < kParts ? wgs : kParts)), dim3(256), 0, st,
                       (const T*)x, R, C, scale, q, qT, parts);
  }
  PA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// slots of the fp32 partials buffer that pa_fp8_amax / pa_fp8_quant fill and pa_fp8_scale_update folds
PA_EXPORT int64_t pa_fp8_nparts() { return kParts; }

// parts[0 : pa_fp8_nparts()] = per-workgroup |x|max of the contiguous x[0 : n] (dtype: common.h DType)
PA_EXPORT int pa_fp8_amax(const void* x, int64_t n, int dtype, float* parts, hipStream_t st) {
  if (n < 0 || !parts) return 1;
  PA_DISPATCH_DTYPE(dtype, T, {
    const int64_t wgs = cdiv(n, 256 * V16<T>::kPer * 4);
    const unsigned grid = (unsigned)(wgs < 1 ? 1 : (wgs < kParts ? wgs : kParts));
    hipLaunchKernelGGL(fp8_amax_k<T>, dim3(grid), dim3(256), 0, st, (const T*)x, n, parts);
  });
  PA_CHECK_LAUNCH();
  return 0;
}

// history: hist_len fp32 (mode 1 only; newest first). scale / scale_inv: one fp32 each, left as they are when the
// amax is 0 or non-finite. fmax: 448 (e4m3fn) / 57344 (e5m2). mode 0 current, 1 delayed.
PA_EXPORT int pa_fp8_scale_update(const float* parts, int n_parts, float* history, int hist_len, float* scale,
                                  float* scale_inv, float fmax, int margin, int mode, hipStream_t st) {
  if (n_parts < 0 || !scale || !scale_inv || mode < 0 || mode > 1 || margin < -64 || margin > 64) return 1;
  if (mode == 1 && (!history || hist_len < 1 || hist_len > 1024)) return 1;
  hipLaunchKernelGGL(fp8_scale_update_k, dim3(1), dim3(256), 0, st, parts, n_parts, history, hist_len, scale,
                     scale_inv, fmax, margin, mode);
  PA_CHECK_LAUNCH();
  return 0;
}

// x [R, C] contiguous (in_dtype: common.h DType) -> q [R, C] = sat(x * *scale) in fmt (0 e4m3fn, 1 e5m2); qT [C, R]
// = q^T when not null; parts (pa_fp8_nparts() fp32) = |x|max partials when not null.
PA_EXPORT int pa_fp8_quant(const void* x, int64_t R, int64_t C, int in_dtype, int fmt, const float* scale, void* q,
                           void* qT, float* parts, hipStream_t st) {
  if (R < 1 || C < 1 || fmt < 0 || fmt > 1 || !scale || !q) return 1;
  PA_DISPATCH_DTYPE(in_dtype, T, {
    return fmt == 0 ? quant_launch<T, 0>(x, R, C, scale, (uint8_t*)q, (uint8_t*)qT, parts, st)
                    : quant_launch<T, 1>(x, R, C, scale, (uint8_t*)q, (uint8_t*)qT, parts, st);
  });
  return 0;
}
