// Device pieces of the OCP MX block rule that more than one file needs: the E8M0 byte of a block from its amax, the
// multiplier that goes with it, the e4m3 conversion, the operand registers of the block-scaled MFMA and the fragment
// reads of its LDS image. mx.hip holds the formats' description; its quantiser and the MoE up projections
// (moe_decode.hip, moe_grouped_mx.hip), which quantise their own output, build a block from these, and mx.hip's tiled
// GEMM and the grouped MoE kernels read the same image, so each rule has one source.
#pragma once
#include "common.h"
#include "mfma_tile.h"

namespace pa {

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int kFmtFp8 = 0, kFmtFp4 = 4;  // the MFMA's cbsz / blgp codes, used as the launchers' format codes

// E8M0 byte of a block with this amax (finite, >= 0): the amax's fp32 exponent field, floor(log2 amax) + 127, minus
// the element format's emax (2 for e2m1, 8 for e4m3); a zero or denormal field clamps to 0, amax == 0 gives 127
template <int EMAX>
__device__ __forceinline__ int mx_block_exp(float amax) {
  const int e = (int)(__float_as_uint(amax) >> 23) - EMAX;
  return amax == 0.f ? 127 : (e < 0 ? 0 : e);
}

// 2^(127 - e), the factor that takes a value to its element, built from bits
__device__ __forceinline__ float mx_block_mult(int e) { return __uint_as_float((uint32_t)(254 - e) << 23); }

__device__ __forceinline__ float sat448(float v) {
  v = v > 448.f ? 448.f : v;
  return v < -448.f ? -448.f : v;
}

// e4m3fn codes of a * s and b * s (saturated, round to nearest even by the hardware convert) in the low (!HI) or
// high (HI) half of `old`
template <bool HI>
__device__ __forceinline__ uint32_t mx_e4m3x2(float a, float b, float s, uint32_t old) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(sat448(a * s), sat448(b * s), (int)old, HI);
}

// MFMA operand registers: an fp4 fragment fills the low four, an fp8 fragment is its two 64-k halves
__device__ __forceinline__ i32x8 widen(uint4 v) {
  i32x8 f = {(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  return f;
}
__device__ __forceinline__ i32x8 join(uint4 lo, uint4 hi) {
  i32x8 f = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  return f;
}

// Fragment reads of a [R][128 B] image. k_swz(row) has period 16 in row, so the lane's byte offset in fragment row
// block i is that of block 0 plus 2048 i (an immediate of the ds_read): `lo` is the offset of row (lane & 15), chunk
// (lane >> 4) ^ k_swz: the fp4 fragment of k-step 0 (k-step 1 is chunk + 4: the offset XOR 64), and the low half of
// an fp8 fragment, whose high half is chunk + 4 of the same image.
__device__ __forceinline__ int frag_lo(int lane, int chunk) {
  const int row = lane & 15;
  return row * 128 + ((chunk ^ k_swz(row)) << 4);
}
__device__ __forceinline__ i32x8 frag4(const char* img, int lo, int s) {
  return widen(*reinterpret_cast<const uint4*>(img + (lo ^ (64 * s))));
}
__device__ __forceinline__ i32x8 frag8(const char* img, int lo) {
  return join(*reinterpret_cast<const uint4*>(img + lo), *reinterpret_cast<const uint4*>(img + (lo ^ 64)));
}

}  // namespace pa
