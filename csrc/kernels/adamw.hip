// Multi-tensor AdamW and Momentum (+ master weights) and multi-tensor sum-of-squares for gfx950.
// Reference behaviour: paddle/phi/kernels/gpu/fused_adam_kernel.cu, adamw_kernel.cu, momentum_kernel.cu.
//
// One launch per parameter group over the table rows and work items of multi_tensor.h (updates: UpdateRow, sum of
// squares: TensorRow). Per element: fp32 math, optional low-precision shadow write in the same pass.
#include "multi_tensor.h"

using namespace pa;

namespace {

// The multi-tensor update kernel: item walk, 4-wide body, scalar tail. Op carries the per-launch scalars and supplies
// kStates (fp32 state tensors per parameter), item(wd, lr_mult) -> the per-item scalars, and update(item, p, st, g):
// one element, p and st[kStates] in place, g the gradient as loaded.
template <typename Op>
__device__ __forceinline__ void update_multi(const int64_t* table, const int64_t* items, int64_t n_items,
                                             const Op& op) {
  constexpr int kS = Op::kStates;
  using Row = UpdateRow<kS>;
  for_each_item<Row>(table, items, n_items, [&](const Row& r, int64_t s, int64_t e) {
    const typename Op::Item item = op.item(r.wd, r.lr_mult);
    int64_t i0 = s;
    if (r.vec4(s)) {  // 4 elements per thread per iteration when everything is aligned
      const int64_t ev = s + ((e - s) / 4) * 4;
      for (int64_t i = s + (int64_t)threadIdx.x * 4; i < ev; i += 256 * 4) {
        float p[4], st[4][kS], g[4];
        V16<float>::ld(r.p + i, p);
        for (int k = 0; k < kS; ++k) {
          const float4 v = *(const float4*)(r.st[k] + i);
          st[0][k] = v.x; st[1][k] = v.y; st[2][k] = v.z; st[3][k] = v.w;
        }
        ld4_any(r.g, i, r.gdt, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) op.update(item, p[j], st[j], g[j]);
        V16<float>::st(r.p + i, p);
        for (int k = 0; k < kS; ++k) *(float4*)(r.st[k] + i) = make_float4(st[0][k], st[1][k], st[2][k], st[3][k]);
        st4_any(r.lp, i, r.ldt, p);
      }
      i0 = ev;
    }
    for (int64_t i = i0 + threadIdx.x; i < e; i += 256) {
      float p = r.p[i], st[kS];
      for (int k = 0; k < kS; ++k) st[k] = r.st[k][i];
      op.update(item, p, st, ld_any(r.g, i, r.gdt));
      for (int k = 0; k < kS; ++k) r.st[k][i] = st[k];
      r.p[i] = p;
      if (r.ldt != kNoShadow) st_any(r.lp, i, r.ldt, p);
    }
  });
}

// AdamW: fp32 math, decoupled weight decay, bias-corrected update; st = {m, v}
struct AdamWOp {
  static constexpr int kStates = 2;
  float inv_scale, lr, b1, b2, eps, bc1, rbc2;
  struct Item { float decay, step; };
  __device__ __forceinline__ Item item(float wd, float lr_mult) const {
    const float plr = lr * lr_mult;
    return {1.f - plr * wd, plr / bc1};
  }
  __device__ __forceinline__ void update(const Item& it, float& p, float* st, float g) const {
    const float gj = g * inv_scale;
    st[0] = b1 * st[0] + (1.f - b1) * gj;
    st[1] = b2 * st[1] + (1.f - b2) * gj * gj;
    p = p * it.decay - it.step * st[0] / (sqrtf(st[1] * rbc2) + eps);
  }
};

// Momentum (paddle/phi/kernels/gpu/momentum_kernel.cu semantics): st = {velocity}; wd = L2 coefficient folded into
// the gradient.
//   g = grad * rescale * inv_scale + wd * p;  vel = mu * vel + g;  p -= lr * (nesterov ? g + mu * vel : vel)
struct MomentumOp {
  static constexpr int kStates = 1;
  float gs, lr, mu;
  int nesterov;
  struct Item { float plr, wd; };
  __device__ __forceinline__ Item item(float wd, float lr_mult) const { return {lr * lr_mult, wd}; }
  __device__ __forceinline__ void update(const Item& it, float& p, float* st, float g) const {
    // g * gs + wd * p with the fused product named: left to the compiler, which of the two products joins the add
    // (and so where the sum is rounded) changed with the surrounding code
    const float gj = __builtin_fmaf(g, gs, it.wd * p);
    st[0] = mu * st[0] + gj;
    p -= it.plr * (nesterov ? gj + mu * st[0] : st[0]);
  }
};

__global__ __launch_bounds__(256) void adamw_multi_k(const int64_t* __restrict__ table, const int64_t* __restrict__ items,
                                                     int64_t n_items, const float* __restrict__ inv_scale_p, float lr,
                                                     float b1, float b2, float eps, float bc1, float bc2,
                                                     const float* __restrict__ hyper) {
  const float inv_scale = inv_scale_p ? *inv_scale_p : 1.f;
  if (hyper) {  // device-resident {lr, beta1^t, beta2^t}: a captured step keeps following the schedule on replay
    lr = hyper[0];
    bc1 = 1.f - hyper[1];
    bc2 = 1.f - hyper[2];
  }
  update_multi(table, items, n_items, AdamWOp{inv_scale, lr, b1, b2, eps, bc1, 1.f / bc2});
}

__global__ __launch_bounds__(256) void momentum_multi_k(const int64_t* __restrict__ table,
                                                        const int64_t* __restrict__ items, int64_t n_items,
                                                        const float* __restrict__ inv_scale_p, float lr, float mu,
                                                        float rescale, int nesterov) {
  update_multi(table, items, n_items, MomentumOp{rescale * (inv_scale_p ? *inv_scale_p : 1.f), lr, mu, nesterov});
}

// partial[blockIdx] = sum of squares of this workgroup's items. The vector body picks its width per item at run
// time inside one loop, so it does not go through the compile-time V16<T>.
__global__ __launch_bounds__(256) void sq_norm_multi_k(const int64_t* __restrict__ table, const int64_t* __restrict__ items,
                                                       int64_t n_items, float* __restrict__ partial) {
  __shared__ float red[4];
  float acc = 0.f;
  for_each_item<TensorRow>(table, items, n_items, [&](const TensorRow& r, int64_t s, int64_t e) {
    const void* X = r.x;
    const int dt = r.dt;
    int64_t i0 = s;
    if ((((uintptr_t)X) & 15) == 0) {  // 16-byte vector path
      const int per = dt == kF32 ? 4 : 8;
      const int64_t ev = s + ((e - s) / per) * per;
      for (int64_t i = s + (int64_t)threadIdx.x * per; i < ev; i += 256 * per) {
        if (dt == kF32) {
          const float4 v = *reinterpret_cast<const float4*>((const float*)X + i);
          acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        } else {
          float v[8];
          if (dt == kBF16) load8<bf16>((const bf16*)X + i, v); else load8<f16>((const f16*)X + i, v);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc += v[j] * v[j];
        }
      }
      i0 = ev;
    }
    for (int64_t i = i0 + threadIdx.x; i < e; i += 256) {
      const float x = ld_any(X, i, dt);
      acc += x * x;
    }
  });
  acc = block_sum<256>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// Values carried as kernel arguments (copied into the launch / the captured graph node at launch time), so a
// pointer table written inside a hipGraph capture does not reference any host buffer on replay.
constexpr int kArgVals = 248;
struct ArgVals {
  int64_t v[kArgVals];
};

__global__ __launch_bounds__(256) void write_i64_k(int64_t* __restrict__ dst, ArgVals a, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = a.v[threadIdx.x];
}

}  // namespace

// elements per work item: the host builds its item lists from this (ops/multi_tensor.py CHUNK)
PA_EXPORT int64_t pa_multi_tensor_chunk() { return kChunk; }

PA_EXPORT int pa_adamw_multi(const int64_t* table, const int64_t* items, int64_t n_items, const float* inv_scale,
                             float lr, float b1, float b2, float eps, float wd_unused, float bc1, float bc2,
                             const float* hyper, hipStream_t st) {
  if (n_items <= 0) return 0;
  hipLaunchKernelGGL(adamw_multi_k, dim3(mt_grid(n_items, 4096)), dim3(256), 0, st, table, items, n_items,
                     inv_scale, lr, b1, b2, eps, bc1, bc2, hyper);
  PA_CHECK_LAUNCH();
  return 0;
}

// One optimizer step of the device-resident Adam hyper-parameters {lr, beta1^t, beta2^t}: the beta powers advance
// on the device (reference: the beta1_pow / beta2_pow accumulators updated inside adam_kernel), so a hipGraph that
// captured the step applies the right bias correction on every replay; lr is written by the LR scheduler.
__global__ void adam_hyper_step_k(float* hyper, float b1, float b2) {
  if (threadIdx.x == 0) {
    hyper[1] *= b1;
    hyper[2] *= b2;
  }
}

PA_EXPORT int pa_adam_hyper_step(float* hyper, float b1, float b2, hipStream_t st) {
  hipLaunchKernelGGL(adam_hyper_step_k, dim3(1), dim3(64), 0, st, hyper, b1, b2);
  PA_CHECK_LAUNCH();
  return 0;
}

// partial must hold 1024 floats; caller sums it.
PA_EXPORT int pa_sq_norm_multi(const int64_t* table, const int64_t* items, int64_t n_items, float* partial,
                               hipStream_t st) {
  (void)hipMemsetAsync(partial, 0, 1024 * sizeof(float), st);
  if (n_items <= 0) return 0;
  hipLaunchKernelGGL(sq_norm_multi_k, dim3(mt_grid(n_items, 1024)), dim3(256), 0, st, table, items, n_items,
                     partial);
  PA_CHECK_LAUNCH();
  return 0;
}

PA_EXPORT int pa_momentum_multi(const int64_t* table, const int64_t* items, int64_t n_items, const float* inv_scale,
                                float lr, float mu, float rescale, int nesterov, hipStream_t st) {
  if (n_items <= 0) return 0;
  hipLaunchKernelGGL(momentum_multi_k, dim3(mt_grid(n_items, 4096)), dim3(256), 0, st, table, items, n_items,
                     inv_scale, lr, mu, rescale, nesterov);
  PA_CHECK_LAUNCH();
  return 0;
}

// dst[0:n] (device) = src[0:n] (host int64), as kernel-argument payloads of <= 248 values per launch.
PA_EXPORT int pa_write_i64(int64_t* dst, const int64_t* src, int64_t n, hipStream_t st) {
  for (int64_t o = 0; o < n; o += kArgVals) {
    ArgVals a;
    const int m = (int)(n - o < kArgVals ? n - o : kArgVals);
    for (int i = 0; i < m; ++i) a.v[i] = src[o + i];
    hipLaunchKernelGGL(write_i64_k, dim3(1), dim3(256), 0, st, dst + o, a, m);
    PA_CHECK_LAUNCH();
  }
  return 0;
}
