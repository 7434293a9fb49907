// Multi-tensor LAMB (+ master weights) for gfx950. Reference behaviour: paddle/phi/kernels/funcs/lamb_functors.h,
// python/paddle/optimizer/lamb.py.
//
// One call per parameter group over the UpdateRow<2> rows (st = {moment1, moment2}) and work items of multi_tensor.h.
// Per element, in fp32:
//   g = grad * inv_scale;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
//   r = (m/bc1) / (sqrt(v/bc2) + eps) + wd*p
//   p -= lr*lr_mult * trust * r,  trust = ||p|| / ||r|| of the whole tensor (1 where the row does not adapt)
// The norms need every element of a tensor before any of its elements may move, so the update is three kernels on one
// stream: lamb_stage1_k writes m and v and one (sum p^2, sum r^2) pair per work item, lamb_trust_k folds the pairs
// of each tensor into its trust ratio, lamb_stage2_k recomputes r from the stored m and v and writes p and the
// low-precision shadow. Every partial has one writer and every sum a fixed order: no atomics, no memset, and two runs
// on the same inputs give the same bits.
#include "multi_tensor.h"

using namespace pa;

namespace {

using Row = UpdateRow<2>;

// the update direction of one element from the moments as stored. Both stages call it on the same p, m and v and must
// get the same bits, so the one product that could be fused into the sum either way is named.
struct LambDir {
  float eps, bc1, bc2;
  __device__ __forceinline__ float operator()(float p, float m, float v, float wd) const {
    return __builtin_fmaf(wd, p, (m / bc1) / (sqrtf(v / bc2) + eps));
  }
};

struct LambMoments {
  float inv_scale, b1, b2;
  __device__ __forceinline__ void operator()(float& m, float& v, float g) const {
    const float gj = g * inv_scale;
    m = b1 * m + (1.f - b1) * gj;
    v = b2 * v + (1.f - b2) * gj * gj;
  }
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block_sum of common.h for a double; blockDim.x == 256, smem holds 4 doubles
__device__ __forceinline__ double block_sum256(double v, double* smem) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

// m, v in place; partial[2*item + {0, 1}] = sum p^2, sum r^2 over the item's elements
__global__ __launch_bounds__(256) void lamb_stage1_k(const int64_t* __restrict__ table,
                                                     const int64_t* __restrict__ items, int64_t n_items,
                                                     float* __restrict__ partial,
                                                     const float* __restrict__ inv_scale_p, float b1, float b2,
                                                     float eps, float bc1, float bc2) {
  __shared__ float red[4];
  const LambMoments moments{inv_scale_p ? *inv_scale_p : 1.f, b1, b2};
  const LambDir dir{eps, bc1, bc2};
  for_each_item_at<Row>(table, items, n_items, [&](const Row& r, int64_t s, int64_t e, int64_t it, int64_t) {
    float sp = 0.f, sr = 0.f;
    int64_t i0 = s;
    if (r.vec4(s)) {
      const int64_t ev = s + ((e - s) / 4) * 4;
      for (int64_t i = s + (int64_t)threadIdx.x * 4; i < ev; i += 256 * 4) {
        float p[4], m[4], v[4], g[4];
        V16<float>::ld(r.p + i, p);
        V16<float>::ld(r.st[0] + i, m);
        V16<float>::ld(r.st[1] + i, v);
        ld4_any(r.g, i, r.gdt, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          moments(m[j], v[j], g[j]);
          const float x = dir(p[j], m[j], v[j], r.wd);
          sp = __builtin_fmaf(p[j], p[j], sp);
          sr = __builtin_fmaf(x, x, sr);
        }
        V16<float>::st(r.st[0] + i, m);
        V16<float>::st(r.st[1] + i, v);
      }
      i0 = ev;
    }
    for (int64_t i = i0 + threadIdx.x; i < e; i += 256) {
      const float p = r.p[i];
      float m = r.st[0][i], v = r.st[1][i];
      moments(m, v, ld_any(r.g, i, r.gdt));
      const float x = dir(p, m, v, r.wd);
      sp = __builtin_fmaf(p, p, sp);
      sr = __builtin_fmaf(x, x, sr);
      r.st[0][i] = m;
      r.st[1][i] = v;
    }
    sp = block_sum<256>(sp, red);
    sr = block_sum<256>(sr, red);
    if (threadIdx.x == 0) {
      partial[it * 2] = sp;
      partial[it * 2 + 1] = sr;
    }
  });
}

// trust[t] for every tensor: one workgroup per tensor folds the partials of its items offsets[t] .. offsets[t + 1],
// in fp64 and in an order fixed by the item count alone. A tensor without items reads nothing and gets 1.
__global__ __launch_bounds__(256) void lamb_trust_k(const int64_t* __restrict__ table,
                                                    const int64_t* __restrict__ offsets, int64_t n_tensors,
                                                    const float* __restrict__ partial, float* __restrict__ trust,
                                                    int always_adapt) {
  __shared__ double red[4];
  for (int64_t t = blockIdx.x; t < n_tensors; t += gridDim.x) {
    const int64_t first = offsets[t], last = offsets[t + 1];
    double sp = 0., sr = 0.;
    for (int64_t it = first + threadIdx.x; it < last; it += 256) {
      sp += (double)partial[it * 2];
      sr += (double)partial[it * 2 + 1];
    }
    sp = block_sum256(sp, red);
    sr = block_sum256(sr, red);
    if (threadIdx.x == 0) {
      const float wd = Row(table + t * Row::kCols).wd;
      trust[t] = ((wd != 0.f || always_adapt) && sp > 0. && sr > 0.) ? (float)(sqrt(sp) / sqrt(sr)) : 1.f;
    }
  }
}

// p -= lr * lr_mult * trust[tensor] * r, r recomputed from the m and v that stage 1 stored; shadow = RNE(p)
__global__ __launch_bounds__(256) void lamb_stage2_k(const int64_t* __restrict__ table,
                                                     const int64_t* __restrict__ items, int64_t n_items,
                                                     const float* __restrict__ trust, float lr, float eps, float bc1,
                                                     float bc2) {
  const LambDir dir{eps, bc1, bc2};
  for_each_item_at<Row>(table, items, n_items, [&](const Row& r, int64_t s, int64_t e, int64_t, int64_t ti) {
    const float step = lr * r.lr_mult * trust[ti];
    int64_t i0 = s;
    if (r.vec4(s)) {
      const int64_t ev = s + ((e - s) / 4) * 4;
      for (int64_t i = s + (int64_t)threadIdx.x * 4; i < ev; i += 256 * 4) {
        float p[4], m[4], v[4];
        V16<float>::ld(r.p + i, p);
        V16<float>::ld(r.st[0] + i, m);
        V16<float>::ld(r.st[1] + i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = __builtin_fmaf(-step, dir(p[j], m[j], v[j], r.wd), p[j]);
        V16<float>::st(r.p + i, p);
        st4_any(r.lp, i, r.ldt, p);
      }
      i0 = ev;
    }
    for (int64_t i = i0 + threadIdx.x; i < e; i += 256) {
      const float p = __builtin_fmaf(-step, dir(r.p[i], r.st[0][i], r.st[1][i], r.wd), r.p[i]);
      r.p[i] = p;
      if (r.ldt != kNoShadow) st_any(r.lp, i, r.ldt, p);
    }
  });
}

}  // namespace

// One LAMB step of a parameter group. offsets: n_tensors + 1 int64, tensor t owns items [offsets[t], offsets[t + 1]);
// partial: 2 * n_items floats of scratch; trust: n_tensors floats, left holding the step's trust ratios.
PA_EXPORT int pa_lamb_multi(const int64_t* table, const int64_t* items, int64_t n_items, const int64_t* offsets,
                            int64_t n_tensors, float* partial, float* trust, const float* inv_scale, float lr, float b1,
                            float b2, float eps, float bc1, float bc2, int always_adapt, hipStream_t st) {
  if (n_tensors <= 0) return 0;
  if (n_items > 0) {
    hipLaunchKernelGGL(lamb_stage1_k, dim3(mt_grid(n_items, 4096)), dim3(256), 0, st, table, items, n_items, partial,
                       inv_scale, b1, b2, eps, bc1, bc2);
    PA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lamb_trust_k, dim3(mt_grid(n_tensors, 1024)), dim3(256), 0, st, table, offsets, n_tensors,
                     partial, trust, always_adapt);
  PA_CHECK_LAUNCH();
  if (n_items > 0) {
    hipLaunchKernelGGL(lamb_stage2_k, dim3(mt_grid(n_items, 4096)), dim3(256), 0, st, table, items, n_items, trust,
                       lr, eps, bc1, bc2);
    PA_CHECK_LAUNCH();
  }
  return 0;
}
