// Weight-only code conversion shared by the kernels that build a bf16 LDS image from int8 / int4 codes
// (moe_grouped_wo.hip, wo_gemm_prefill.hip): 16 codes along K of one 16-byte load -> the two 16-byte chunks of a
// K-major image row. int4 is weight_quantize's pair-row byte: channel 2j in the low nibble, 2j + 1 in the high one,
// stored + 8, all 16 codes decode.
#pragma once
#include "common.h"

namespace pa {

// two small integers as a bf16 pair: exact, so the high halves of the floats are the bf16 bits
__device__ __forceinline__ uint32_t gwo_bf16x2(int a, int b) {
  return __builtin_amdgcn_perm(__float_as_uint((float)b), __float_as_uint((float)a), 0x07060302u);
}

// the 4 codes of dword u (int4: already XORed with 0x88888888) as signed integers. Per element one signed bit-field
// extract; HI: the high nibbles.
template <int BITS, bool HI>
__device__ __forceinline__ void gwo_codes4(uint32_t u, int* v) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int pos = 8 * b + (BITS == 4 && HI ? 4 : 0);
    v[b] = (int)(u << (32 - BITS - pos)) >> (32 - BITS);
  }
}

// 16 codes along K -> 16 bf16 as the two 16-byte chunks of the image (k 0 .. 7, k 8 .. 15). Per element one signed
// bit-field extract, one convert and half a byte permute; int4 flips every nibble's top bit first (one XOR a dword),
// which turns the stored code c = v + 8 into v's 4-bit two's complement. HI: the high nibbles.
template <int BITS, bool HI>
__device__ __forceinline__ void gwo_cvt(const uint4& raw, uint4& c0, uint4& c1) {
  const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    int v[4];
    gwo_codes4<BITS, HI>(BITS == 8 ? wd[w] : wd[w] ^ 0x88888888u, v);
    o[2 * w] = gwo_bf16x2(v[0], v[1]);
    o[2 * w + 1] = gwo_bf16x2(v[2], v[3]);
  }
  c0 = make_uint4(o[0], o[1], o[2], o[3]);
  c1 = make_uint4(o[4], o[5], o[6], o[7]);
}

// The same with a group scale: every element is bf16(code * s), rounded to nearest even by v_cvt_pk_bf16_f32, which
// is the element pa_wo_dequant writes.
template <int BITS, bool HI>
__device__ __forceinline__ void gwo_cvt_scaled(const uint4& raw, float s, uint4& c0, uint4& c1) {
  const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    int v[4];
    gwo_codes4<BITS, HI>(BITS == 8 ? wd[w] : wd[w] ^ 0x88888888u, v);
    o[2 * w] = pack_bf16((float)v[0] * s, (float)v[1] * s);
    o[2 * w + 1] = pack_bf16((float)v[2] * s, (float)v[3] * s);
  }
  c0 = make_uint4(o[0], o[1], o[2], o[3]);
  c1 = make_uint4(o[4], o[5], o[6], o[7]);
}

}  // namespace pa
