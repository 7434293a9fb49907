// What the MoE decode kernels (moe_decode.hip) and the grouped MXFP4 prefill kernels (moe_grouped_mx.hip) share: the
// argument block of the bf16 decode FFN, SwiGLU's silu, and the combine kernel that ends both paths. One definition,
// so both paths sum a token's experts in the same order.
#pragma once
#include "common.h"

namespace pa {
namespace {

struct MoeDecArgs {
  const uint16_t *x, *w1, *w2, *b1, *b2;
  const float* val;
  const int *idx, *offs, *perm, *pos, *active, *n_active;
  uint16_t* h;    // [n, f] bf16, sorted row order
  float* ws;      // [splits, n, d] fp32
  uint16_t* out;  // [T, d] bf16
  int T, E, topk, d, f, n, k_per, splits;
};

__device__ __forceinline__ float silu(float a) { return a / (1.f + __expf(-a)); }

// out[t][c] = sum_j val[t, j] * (sum_s slab[s][pos[t topk + j]][c] + b2[idx[t, j]][c]), j and s ascending
__global__ __launch_bounds__(256) void moe_decode_combine_k(MoeDecArgs p) {
  const int t = blockIdx.y;
  const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (c >= p.d) return;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < p.topk; ++j) {
    const int ent = t * p.topk + j;
    const int row = min(max(p.pos[ent], 0), p.n - 1);
    float4 s = *reinterpret_cast<const float4*>(p.ws + (int64_t)row * p.d + c);
    for (int sp = 1; sp < p.splits; ++sp) {
      const float4 u = *reinterpret_cast<const float4*>(p.ws + ((int64_t)sp * p.n + row) * p.d + c);
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
    }
    if (p.b2) {
      float b[4];
      const int e = min(max(p.idx[ent], 0), p.E - 1);
      load4_16(p.b2 + (int64_t)e * p.d + c, b);
      s.x += b[0]; s.y += b[1]; s.z += b[2]; s.w += b[3];
    }
    const float w = p.val[ent];
    o[0] += w * s.x; o[1] += w * s.y; o[2] += w * s.z; o[3] += w * s.w;
  }
  *reinterpret_cast<uint2*>(p.out + (int64_t)t * p.d + c) = make_uint2(pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]));
}

}  // namespace
}  // namespace pa
