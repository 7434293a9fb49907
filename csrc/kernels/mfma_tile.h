// LDS tile primitives of the MFMA kernels (gemm.hip, grouped_gemm.hip, gemm_fp8.hip, gemm_skinny.hip,
// flash_attn_kernels.h): LDS-DMA, the transposing LDS read, counted waits, the fenced barrier, the image
// swizzles with the stage / fragment-read pair each one binds, and the tile order. One definition each:
// the stage side and the read side of a swizzle cannot drift apart between files. The schedule built from them
// for the 256x256 ping-pong kernels (gemm256_kernel, gemm_fp8_pp_kernel) is one level up, in pingpong256.h.
#pragma once
#include "common.h"

namespace pa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// one 16x16x32 bf16 MFMA operand (8 values per lane) and its load views
union Frag8 {
  bf16x8_t v;
  uint4 u;
  u32x4 w;
  s16x4 h[2];
};

// global_load_lds issued from inline asm: hipcc treats a builtin LDS-DMA as a pending write to
// every LDS object and puts s_waitcnt vmcnt(0) in front of the next ds_read, which would drain the
// prefetch pipeline each phase. The kernels retire the DMA themselves with counted vmcnt + barrier.
// M0 holds the wave-uniform LDS destination (lane i writes base + 16 i).
__device__ __forceinline__ void glds16(const void* g, const char* lds_wave_base) {
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(lds_wave_base));
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(m0) : "memory", "m0");
}
// the 4-byte form (lane i writes base + 4 i)
__device__ __forceinline__ void glds4(const void* g, const char* lds_wave_base) {
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(lds_wave_base));
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g), "s"(m0) : "memory", "m0");
}

// ds_read_b64_tr_b16: the hardware-transposed read of MN-major (row = k) images
__device__ __forceinline__ s16x4 lds_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(reinterpret_cast<uintptr_t>(p)));
}

// workgroup barrier that waits for no counter and that the scheduler moves nothing across
__device__ __forceinline__ void bar() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the immediate must be a literal)
__device__ __forceinline__ void vm_wait(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// ---- swizzles: an XOR on the 16-B chunk index of an image row. glds writes LDS lane-linearly, so the stage
// side applies the swizzle to the per-lane GLOBAL source address and the fragment read undoes it on the LDS
// address: both sides of a pair, or neither.
// K-major images with 128-B rows ([R][64] 16-bit, [R][128] fp8): stage<R, true> and the conv gathers of
// gemm.hip write it; frag<R, true> and gemm_fp8.hip's frag read it.
constexpr __host__ __device__ __forceinline__ int k_swz(int row) { return (row >> 1) & 7; }
// K-major images with 64-B rows ([R][32]): Loader32<true> / frag32<true> of gemm.hip, the dS image of
// fa_bwd_dq_kernel. Also the whole XOR of gemm.hip's MN-major [64][160] image (mn_swz3: stage_r / frag_r).
constexpr __host__ __device__ __forceinline__ int k32_swz(int row) { return ((row >> 3) & 1) << 1; }
// MN-major images ([k][R], R >= 128), an even XOR so 32-B pairs stay together: the conv weight-gradient
// gather and Loader32<false> of gemm.hip write it for frag<256, false>, fa_bwd_dq_kernel for its dq_frag.
constexpr __host__ __device__ __forceinline__ int mn_swz(int k) { return ((k & 3) | (((k >> 3) & 1) << 2)) << 1; }
// mn_swz for a k-row of R columns (R / 8 chunks): stage<R, false> and grouped_gemm.hip's stage_mn write it,
// frag<R, false> reads it, for R = 64, 128, 256. A no-op for R >= 128; R = 64 keeps the chunk inside its row.
template <int R>
constexpr __host__ __device__ __forceinline__ int mn_swz_r(int k) { return mn_swz(k) & (R / 8 - 1); }

// The XOR is even and, being injective, a bijection chunk -> slot of a k-row if no slot leaves the row; for
// R >= 128 the mask changes nothing (mn_swz < 16).
template <int R>
constexpr bool mn_swz_ok() {
  for (int k = 0; k < 64; ++k) {
    const int s = mn_swz_r<R>(k);
    if (s % 2 != 0 || (R >= 128 && s != mn_swz(k))) return false;
    for (int c = 0; c < R / 8; ++c)
      if ((c ^ s) >= R / 8) return false;
  }
  return true;
}
static_assert(mn_swz_ok<64>() && mn_swz_ok<128>() && mn_swz_ok<256>(), "MN-major swizzle");

// ---- staging of one operand tile (R rows of the output dimension x 128 bytes of k) into LDS with glds16
// K-major: image [R][128 B], rows past rmax clamped.  MN-major (16-bit only): image [64][R], columns clamped.
// NW waves share the R / 8 wave-instructions of 1 KiB (R a multiple of 8 NW; gemm.hip's stage_r covers R = 160).
template <int R, bool KMAJ, int NW = 8, class T>
__device__ __forceinline__ void stage(const T* __restrict__ g, int64_t ld, int r0, int rmax, int k0, char* img,
                                      int wave, int lane) {
  constexpr int E = 16 / sizeof(T);  // elements per chunk
  constexpr int NQ = R / (8 * NW);   // glds instructions per thread
  static_assert(KMAJ || sizeof(T) == 2, "MN-major images hold 16-bit elements");
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int q = i * NW + wave;  // wave-instruction id
    if constexpr (KMAJ) {
      const int row = q * 8 + (lane >> 3);  // 8 rows x 128 B
      const int lc = (lane & 7) ^ k_swz(row);
      int gr = r0 + row;
      gr = gr < rmax ? gr : rmax - 1;
      glds16(g + (int64_t)gr * ld + k0 + lc * E, img + q * 1024);
    } else {
      constexpr int CPR = R / 8;  // chunks per k-row
      const int lin = q * 64 + lane;
      const int row = lin / CPR;  // k
      const int lc = (lin % CPR) ^ mn_swz_r<R>(row);
      int gc = r0 + lc * 8;
      gc = gc < rmax ? gc : rmax - 8;
      glds16(g + (int64_t)(k0 + row) * ld + gc, img + q * 1024);
    }
  }
}

// ---- fragment read of a 16-bit image: 16 rows (output dim) x 8 k for k-substep s (32 k) -> mfma operand
template <int R, bool KMAJ>
__device__ __forceinline__ bf16x8_t frag(const char* img, int rbase, int s, int lane) {
  Frag8 f;
  if constexpr (KMAJ) {
    const int row = rbase + (lane & 15);
    const int c = s * 4 + (lane >> 4);
    f.u = *reinterpret_cast<const uint4*>(img + row * 128 + ((c ^ k_swz(row)) << 4));
  } else {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
    const int col = rbase + pp * 4;  // first of 4 columns supplied by this lane
    const int lc = col >> 3, sub = (col & 7) * 2;
    const int k1 = s * 32 + g * 8 + q, k2 = k1 + 4;
    f.h[0] = lds_tr(img + k1 * (R * 2) + ((lc ^ mn_swz_r<R>(k1)) << 4) + sub);
    f.h[1] = lds_tr(img + k2 * (R * 2) + ((lc ^ mn_swz_r<R>(k2)) << 4) + sub);
  }
  return f.v;
}

// ---- tile order
// XCD-aware bijective remap: workgroup ids are dealt round-robin over the 8 XCDs; each XCD gets a contiguous
// run of tiles, so the blocks of one XCD share operand panels in their private L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// grouped tile order (8 m-tiles per group, so neighbouring workgroups share B panels)
__device__ __forceinline__ void tile_coords(int pid, int tiles_m, int tiles_n, int* tm, int* tn) {
  constexpr int GM = 8;
  const int per_group = GM * tiles_n;
  const int first_m = (pid / per_group) * GM;
  const int gsz = min(tiles_m - first_m, GM);
  *tm = first_m + (pid % per_group) % gsz;
  *tn = (pid % per_group) / gsz;
}

// a compile-time int passed as a value (generic lambdas that specialise a K-loop body)
template <int V>
struct IntC {
  static constexpr int value = V;
};

}  // namespace pa
