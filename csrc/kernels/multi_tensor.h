// The multi-tensor scheme of the optimizer updates, the sum of squares (adamw.hip) and the unscale pass (amp.hip).
// The host (ops/multi_tensor.py) uploads a table of int64 rows, one per tensor (TensorRow or UpdateRow), and work
// items (2 x int64): [tensor index, start element]; each item covers kChunk elements. A persistent grid of 256-thread
// workgroups walks the items; inside an item: a 16-byte vector body where the pointers allow it, then a scalar tail.
#pragma once
#include "common.h"

namespace pa {

constexpr int64_t kChunk = 16384;  // elements per work item; start elements are multiples of it
constexpr int kNoShadow = 3;       // low-precision dtype code of an update row without a shadow copy

// workgroups of a persistent launch: one per item up to the kernel's cap
inline unsigned mt_grid(int64_t n_items, int64_t cap) { return (unsigned)(n_items < cap ? n_items : cap); }

// [ptr, numel, dtype]
struct TensorRow {
  static constexpr int kCols = 3, kNumelCol = 1;
  void* x;
  int dt;
  __device__ __forceinline__ explicit TensorRow(const int64_t* r) : x((void*)r[0]), dt((int)r[2]) {}
};

// [param_fp32*, grad*, state0*, state1*, lowp_param* (or 0), numel, gdtype | (ldtype << 8), wd (f32 bits),
//  lr_mult (f32 bits)]; an update with one state tensor leaves the state1 column unread
template <int kStates> struct UpdateRow {
  static constexpr int kCols = 9, kNumelCol = 5;
  float *p, *st[kStates];
  const void* g;
  void* lp;
  int gdt, ldt;
  float wd, lr_mult;
  __device__ __forceinline__ explicit UpdateRow(const int64_t* r)
      : p((float*)r[0]), g((const void*)r[1]), lp((void*)r[4]), gdt((int)(r[6] & 0xff)), ldt((int)((r[6] >> 8) & 0xff)),
        wd(__int_as_float((int)r[7])), lr_mult(__int_as_float((int)r[8])) {
    for (int k = 0; k < kStates; ++k) st[k] = (float*)r[2 + k];
  }
  // the item starting at element s may take the 4-wide body: 16-byte fp32 accesses, 8-byte 16-bit ones
  __device__ __forceinline__ bool vec4(int64_t s) const {
    uintptr_t f32 = (uintptr_t)p;
    for (int k = 0; k < kStates; ++k) f32 |= (uintptr_t)st[k];
    return ((f32 & 15) == 0) && ((((uintptr_t)g) & (gdt == kF32 ? 15 : 7)) == 0) &&
           (ldt == kNoShadow || ((((uintptr_t)lp) & (ldt == kF32 ? 15 : 7)) == 0)) && (s % 4 == 0);
  }
};

// body(row, s, e, it, ti) for every item of this workgroup: elements [s, e) of the tensor that `row` describes, item
// number `it` of the work list, tensor number `ti` of the table
template <typename Row, typename Body>
__device__ __forceinline__ void for_each_item_at(const int64_t* table, const int64_t* items, int64_t n_items,
                                                 Body&& body) {
  for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int64_t ti = items[it * 2], s = items[it * 2 + 1];
    const int64_t* r = table + ti * Row::kCols;
    const int64_t n = r[Row::kNumelCol];
    body(Row(r), s, s + kChunk < n ? s + kChunk : n, it, ti);
  }
}

// body(row, s, e): the same walk for a body that needs neither number
template <typename Row, typename Body>
__device__ __forceinline__ void for_each_item(const int64_t* table, const int64_t* items, int64_t n_items,
                                              Body&& body) {
  for_each_item_at<Row>(table, items, n_items,
                        [&](const Row& r, int64_t s, int64_t e, int64_t, int64_t) { body(r, s, e); });
}

__device__ __forceinline__ float ld_any(const void* p, int64_t i, int dt) {
  if (dt == kF32) return ((const float*)p)[i];
  if (dt == kBF16) return to_f(((const bf16*)p)[i]);
  return to_f(((const f16*)p)[i]);
}

__device__ __forceinline__ void st_any(void* p, int64_t i, int dt, float x) {
  if (dt == kF32) ((float*)p)[i] = x;
  else if (dt == kBF16) ((bf16*)p)[i] = from_f<bf16>(x);
  else ((f16*)p)[i] = from_f<f16>(x);
}

// one 16-byte access per lane: 4 x fp32 or 8 x bf16 / fp16
template <typename T> struct V16 {
  static constexpr int kPer = 8;
  static __device__ __forceinline__ void ld(const T* p, float* f) { load8<T>(p, f); }
  static __device__ __forceinline__ void st(T* p, const float* f) { store8<T>(p, f); }
};
template <> struct V16<float> {
  static constexpr int kPer = 4;
  static __device__ __forceinline__ void ld(const float* p, float* f) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* f) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};

// f[0:4] = p[i:i+4] as fp32: one 16-byte (fp32) or 8-byte (bf16 / fp16) load
__device__ __forceinline__ void ld4_any(const void* p, int64_t i, int dt, float* f) {
  if (dt == kF32) return V16<float>::ld((const float*)p + i, f);
  const uint2 w = *(const uint2*)((const uint16_t*)p + i);
  if (dt == kBF16) { f[0] = lo_bf16(w.x); f[1] = hi_bf16(w.x); f[2] = lo_bf16(w.y); f[3] = hi_bf16(w.y); }
  else { f[0] = lo_f16(w.x); f[1] = hi_f16(w.x); f[2] = lo_f16(w.y); f[3] = hi_f16(w.y); }
}

// p[i:i+4] = f[0:4] rounded to dt; nothing for kNoShadow
__device__ __forceinline__ void st4_any(void* p, int64_t i, int dt, const float* f) {
  if (dt == kBF16) *(uint2*)((uint16_t*)p + i) = make_uint2(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]));
  else if (dt == kF16) *(uint2*)((uint16_t*)p + i) = make_uint2(pack_f16(f[0], f[1]), pack_f16(f[2], f[3]));
  else if (dt == kF32) V16<float>::st((float*)p + i, f);
}

}  // namespace pa
