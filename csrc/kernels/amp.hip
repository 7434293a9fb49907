// Multi-tensor non-finite check + unscale of gradients (loss scaling) for gfx950.
// Reference behaviour: paddle/phi/kernels/gpu/amp_kernel.cu (check_finite_and_unscale).
//
// Table rows (TensorRow) and work items of multi_tensor.h, as in sq_norm_multi_k (adamw.hip).
// Per element: x loaded as fp32, y = x * *inv_scale stored back in the tensor's own dtype. One launch covers
// fp32 / bf16 / fp16 tensors together. found_inf[0] is set to 1 when any loaded value is inf or nan; it is never
// cleared here, so calls accumulate.
#include "multi_tensor.h"

using namespace pa;

namespace {

constexpr int kUnroll = 4;  // 16-byte requests in flight per lane in the vector body

// exponent all ones, tested on the bits: holds whatever floating-point flags the file is built with
__device__ __forceinline__ int non_finite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// elements [s, e) of X in place; returns 1 if this thread loaded a non-finite value
template <typename T>
__device__ __forceinline__ int unscale_item(T* X, int64_t s, int64_t e, float inv) {
  constexpr int P = V16<T>::kPer;
  constexpr int64_t kStride = 256 * P;
  int bad = 0;
  int64_t i0 = s;
  if ((((uintptr_t)X) & 15) == 0) {  // s is a multiple of kChunk, so X + s keeps the 16-byte alignment of X
    const int64_t ev = s + ((e - s) / P) * P;
    int64_t i = s + (int64_t)threadIdx.x * P;
    // all loads of a trip are issued before its first store (the update is in place: the compiler cannot hoist them)
    for (; i + (kUnroll - 1) * kStride < ev; i += kUnroll * kStride) {
      float v[kUnroll][P];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) V16<T>::ld(X + i + u * kStride, v[u]);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
          bad |= non_finite(v[u][j]);
          v[u][j] *= inv;
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) V16<T>::st(X + i + u * kStride, v[u]);
    }
    for (; i < ev; i += kStride) {
      float v[P];
      V16<T>::ld(X + i, v);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        bad |= non_finite(v[j]);
        v[j] *= inv;
      }
      V16<T>::st(X + i, v);
    }
    i0 = ev;
  }
  for (int64_t i = i0 + threadIdx.x; i < e; i += 256) {  // scalar tail (whole item when X is not 16-byte aligned)
    const float x = to_f(X[i]);
    bad |= non_finite(x);
    X[i] = from_f<T>(x * inv);
  }
  return bad;
}

__global__ __launch_bounds__(256) void amp_check_unscale_multi_k(const int64_t* __restrict__ table,
                                                                 const int64_t* __restrict__ items, int64_t n_items,
                                                                 const float* __restrict__ inv_scale,
                                                                 float* __restrict__ found_inf) {
  const float inv = *inv_scale;
  int bad = 0;
  // for_each_item<TensorRow> written out: through its lambda the compiler lays this kernel out differently (17 more
  // instructions), and that code did not stay inside the parent's timing spread in every run
  for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int64_t ti = items[it * 2], s = items[it * 2 + 1];
    const int64_t* row = table + ti * TensorRow::kCols;
    const TensorRow r(row);
    const int64_t n = row[TensorRow::kNumelCol];
    const int64_t e = s + kChunk < n ? s + kChunk : n;
    if (r.dt == kF32) bad |= unscale_item<float>((float*)r.x, s, e, inv);
    else if (r.dt == kBF16) bad |= unscale_item<bf16>((bf16*)r.x, s, e, inv);
    else if (r.dt == kF16) bad |= unscale_item<f16>((f16*)r.x, s, e, inv);
  }
  // every writer stores the same value: no atomic needed
  if (__syncthreads_or(bad) && threadIdx.x == 0) found_inf[0] = 1.0f;
}

}  // namespace

// found_inf is not cleared: the caller zeroes it once and may check several gradient sets into it.
PA_EXPORT int pa_amp_check_unscale_multi(const int64_t* table, const int64_t* items, int64_t n_items,
                                         const float* inv_scale, float* found_inf, hipStream_t st) {
  if (n_items <= 0) return 0;
  hipLaunchKernelGGL(amp_check_unscale_multi_k, dim3(mt_grid(n_items, 1024)), dim3(256), 0, st, table, items,
                     n_items, inv_scale, found_inf);
  PA_CHECK_LAUNCH();
  return 0;
}
