// The 256x256 8-wave ping-pong schedule, once, for every operand width (gemm.hip gemm256_kernel: bf16, K-tiles of
// 64; gemm_fp8.hip gemm_fp8_pp_kernel: fp8, K-tiles of 128; either way a K-tile row is 128 bytes).
//
// Every K-tile is split into four 16-KiB half-tiles
//   H0 = A rows 0..127, H1 = B cols 0..127, H2 = A rows 128..255, H3 = B cols 128..255
// and each of its four phases is {ds_read a register subtile ; issue ONE half-tile of glds ; barrier ; MFMA
// cluster ; barrier}. Reads: phase 0 H0+H1, phase 1 H3, phase 2 H2. Half-tile j (= 4 * tile + h) is issued in
// phase j - 6, so 5-6 phases of load latency are hidden, and each read is preceded by a counted vmcnt
// in the phase before it. The wm == 1 waves run one barrier behind the wm == 0 waves (ping-pong:
// per SIMD one wave is in its MFMA cluster while the other reads LDS / issues glds); because of the
// stagger a half-tile is restaged at least two phases after its last ds_read (WAR), and a read
// happens at least one barrier after the wait that retires it in both wave groups (RAW).
// Wave (wm, wn) owns rows {wm*64.., 128+wm*64..} x cols {wn*32.., 128+wn*32..}: the four phases
// compute its quadrants (top,L) (top,R) (bottom,L) (bottom,R) into acc[row half][4][column half][2].
//
// What differs between the operand widths is the policy `Ops` of PPLoop: the fragment type and its LDS
// read, the MFMA, and how a half-tile is staged. The tail-slice decode, the raw partial store of a tail slice,
// the sum of the partials and the one-pass 16-bit epilogue are shared as well.
#pragma once
#include "mfma_tile.h"

namespace pa {

constexpr int kPPThreads = 512;
constexpr int kPPHalf = 128 * 128;        // a half-tile: 128 rows x 128 bytes of k (16 KiB)
constexpr int kPPStage = 4 * kPPHalf;     // one K-tile
constexpr int kPPLoopLds = 2 * kPPStage;  // two stages (128 KiB)
constexpr int kPPEpiRow16 = 264;          // 16-bit values per row of the one-pass epilogue image (528-byte rows)
constexpr int kPPEpiLds16 = 256 * kPPEpiRow16 * 2;
constexpr int kPPLds16 = kPPLoopLds > kPPEpiLds16 ? kPPLoopLds : kPPEpiLds16;  // loop, then the 16-bit epilogue
constexpr int kPPTileElems = 256 * 256;   // fp32 values of a tail slice's partial

// Balanced tail: the first full_tiles workgroups (a whole number of waves over the CUs) own whole
// tiles; the remaining tiles are cut along K so the last wave is as wide as the chip (320 tiles of a
// 4096 x 5120 output on 256 CUs: 256 whole + 64 x 4 quarter tiles = 1.25 tile-times instead of 2).
// Workgroup bid -> tile pid; for a tail slice also its K slice ks, its partial tail_out (else null), and p.K
// becomes the slice's K. The caller moves its operand bases (or its first K-tile) by ks slices.
struct PPWork {
  int pid, ks;
  float* tail_out;
};
template <class Args>
__device__ __forceinline__ PPWork pp_work(Args& p, int bid) {
  PPWork w{0, 0, nullptr};
  if (p.tail_split > 0 && bid >= p.full_tiles) {
    const int u = bid - p.full_tiles;
    w.ks = u % p.tail_split;
    w.pid = p.full_tiles + u / p.tail_split;
    p.K /= p.tail_split;
    w.tail_out = p.tail_ws + (int64_t)u * kPPTileElems;
  } else {
    w.pid = xcd_remap(bid, p.tail_split > 0 ? p.full_tiles : p.tiles_m * p.tiles_n);
  }
  return w;
}

// The main loop over nk K-tiles: prologue, one K-tile of four phases, closing barrier. Ops supplies
//   kSub                          k-substeps (MFMAs per fragment pair) of a K-tile
//   Frag                          one MFMA operand
//   stage_half(t, h, dst)         glds of half h of local K-tile t into the 16-KiB image dst
//   read_a / read_b(img, rbase, ks, lane)   fragment of 16 rows from rbase of a half-tile image, substep ks
//   mma(b, a, c)                  c += b x a (operands swapped: a lane ends with 4 consecutive columns of a row)
// A kernel runs it as
//   PPLoop<Ops> L{ops, smem, nk, wm, wn, lane, acc};
//   L.start();
//   int t = 0;
//   for (; t < L.nsteady(); ++t) L.ktile(t, IntC<1>{});   // both loops "#pragma unroll 1"
//   for (; t < nk; ++t) L.ktile(t, IntC<0>{});
//   L.finish();
// The two loops stay in the kernel on purpose. The compiler optimises a callee on its own before it inlines it,
// and with the loops inside a function here it no longer turned the staging addresses into per-lane pointers
// plus one scalar offset per K-tile: the steady loop of gemm256_kernel<false, false, 0> grew from 215 to 250
// instructions (per-lane 64-bit multiplies) and bf16 ran 2 - 9 % slower (profiles/pingpong_single_source.md).
template <class Ops>
struct PPLoop {
  using Frag = typename Ops::Frag;
  static constexpr int KS = Ops::kSub;
  const Ops& ops;
  char* smem;
  int nk, wm, wn, lane;
  f32x4 (&acc)[2][4][2][2];
  int last_j, ar, bc;
  bool lag;
  Frag af[4][KS], bl[2][KS], br[2][KS];

  // issue half-tile j (tile j>>2, half j&3) into buffer (j>>2)&1
  __device__ void issue(int j) const {
    const int t = j >> 2, h = j & 3;
    ops.stage_half(t, h, smem + (t & 1) * kPPStage + h * kPPHalf);
  }
  // the same with the half known at compile time (steady-state body: no branch on h)
  template <class HC>
  __device__ void issue_h(int t, HC) const {
    constexpr int h = HC::value;
    ops.stage_half(t, h, smem + (t & 1) * kPPStage + h * kPPHalf);
  }
  // Half-tile j is issued in phase j - 6 (phase = 4 * tile + p). Before each phase that reads a
  // half-tile the waves wait (in the previous phase, before its first barrier) until that half-tile
  // is retired: vmcnt = 2 * (half-tiles issued after it).
  __device__ void wait_for(int phase, int jstar) const {
    const int issued = min(phase + 6, last_j);
    vm_wait(2 * max(issued - jstar, 0));
  }
  __device__ int nsteady() const { return max(nk - 2, 0); }

  // zero the accumulators, issue the first six half-tiles, wait for H0 / H1 of tile 0, start the stagger
  __device__ void start() {
    last_j = 4 * nk - 1;
    ar = wm * 64;
    bc = wn * 32;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[a][i][b][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int npro = min(6, 4 * nk);
#pragma unroll 1
    for (int j = 0; j < npro; ++j) issue(j);
    vm_wait(2 * max(min(5, last_j) - 1, 0));  // H0, H1 of tile 0
    bar();
    // ping-pong: the wm == 1 waves run one barrier behind, so on every SIMD one wave issues its
    // MFMA cluster while the other does its ds_reads / glds (+1 barrier at the end for wm == 0).
    lag = __builtin_amdgcn_readfirstlane(wm) == 1;
    if (lag) bar();
  }
  __device__ void finish() const {
    if (!lag) bar();
  }

  // the MFMA cluster of one phase, quadrant (a, b): ks outermost, so no two MFMAs on one accumulator are adjacent
  template <class AC, class BC>
  __device__ void cluster(AC, BC, const Frag (&bf)[2][KS]) {
    constexpr int a = AC::value, b = BC::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][i][b][j] = Ops::mma(bf[j][ks], af[i][ks], acc[a][i][b][j]);
    __builtin_amdgcn_s_setprio(0);
  }

  // One K-tile = 4 phases. STEADY (t <= nk - 3): every issue happens and every wait count is the
  // constant of the formula above (issued - jstar = 3, 5, 4 half-tiles -> vmcnt 6, 10, 8), so the body
  // has no branches; the last two tiles run the generic body with clamped counts.
  template <class ST>
  __device__ void ktile(int t, ST) {
    constexpr bool S = ST::value;
    const char* buf = smem + (t & 1) * kPPStage;
    const int ph = 4 * t;
    // ---- phase 0: read A-top + B-left; issue j = ph + 6; MFMA (top, L)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) bl[j][ks] = Ops::read_b(buf + kPPHalf, bc + j * 16, ks, lane);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i][ks] = Ops::read_a(buf, ar + i * 16, ks, lane);
    if (S) {
      issue_h(t + 1, IntC<2>{});
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // B-right of this tile, read in phase 1
    } else {
      if (ph + 6 <= last_j) issue(ph + 6);
      wait_for(ph, ph + 3);
    }
    bar();
    cluster(IntC<0>{}, IntC<0>{}, bl);
    bar();
    // ---- phase 1: read B-right; issue j = ph + 7; MFMA (top, R)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) br[j][ks] = Ops::read_b(buf + 3 * kPPHalf, bc + j * 16, ks, lane);
    if (S) {
      issue_h(t + 1, IntC<3>{});
      asm volatile("s_waitcnt vmcnt(10)" ::: "memory");  // A-bottom of this tile, read in phase 2
    } else {
      if (ph + 7 <= last_j) issue(ph + 7);
      wait_for(ph + 1, ph + 2);
    }
    bar();
    cluster(IntC<0>{}, IntC<1>{}, br);
    bar();
    // ---- phase 2: read A-bottom; issue j = ph + 8; MFMA (bottom, L)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i][ks] = Ops::read_a(buf + 2 * kPPHalf, ar + i * 16, ks, lane);
    if (S) issue_h(t + 2, IntC<0>{});
    else if (ph + 8 <= last_j) issue(ph + 8);
    bar();
    cluster(IntC<1>{}, IntC<0>{}, bl);
    bar();
    // ---- phase 3: issue j = ph + 9; wait for H0/H1 of tile t+1; MFMA (bottom, R)
    if (S) {
      issue_h(t + 2, IntC<1>{});
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      if (ph + 9 <= last_j) issue(ph + 9);
      if (t + 1 < nk) wait_for(ph + 3, ph + 5);
    }
    bar();
    cluster(IntC<1>{}, IntC<1>{}, br);
    bar();
  }
};

// K-slice of a tail tile: the raw fp32 partial, row-major 256 x 256
__device__ __forceinline__ void pp_store_partial(float* tail_out, const f32x4 (&acc)[2][4][2][2], int wm, int wn,
                                                 int lane) {
  const int ar = wm * 64, bc = wn * 32;
#pragma unroll
  for (int bh = 0; bh < 2; ++bh)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ah = 0; ah < 2; ++ah)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = ah * 128 + ar + i * 16 + (lane & 15);
          const int c = bh * 128 + bc + j * 16 + 4 * (lane >> 4);
          const f32x4 v = acc[ah][i][bh][j];
          *reinterpret_cast<float4*>(tail_out + r * 256 + c) = make_float4(v[0], v[1], v[2], v[3]);
        }
}

// sum of the `split` partials of 4 consecutive elements (src: the element in slice 0 of the tile's partials)
__device__ __forceinline__ float4 tail_sum4(const float* src, int split) {
  float4 a = *reinterpret_cast<const float4*>(src);
  for (int k = 1; k < split; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)k * kPPTileElems);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  return a;
}

// One-pass epilogue of a 16-bit output: pack(elem(acc * alpha + bias)) in registers, the finished tile staged
// through LDS ([256][kPPEpiRow16] 16-bit, reusing the loop's stages: every glds must be retired), then 16-byte
// row stores of whole 512-byte row segments (N % 8 == 0, ldc % 8 == 0).
//   bias4(n, bq)   the bias of columns n..n+3 into bq (preset to 0; n may be past N)
//   elem(v)        the activation;  pack(a, b)  two values -> one 32-bit word of the output type
template <class Bias4, class Elem, class Pack>
__device__ __forceinline__ void pp_epilogue16(char* smem, const f32x4 (&acc)[2][4][2][2], uint16_t* c, int64_t ldc,
                                              int M, int N, int m0, int n0, float alpha, int tid, Bias4 bias4,
                                              Elem elem, Pack pack) {
  const int wave = tid >> 6, lane = tid & 63;
  const int ar = (wave >> 2) * 64, bc = (wave & 3) * 32;
  uint16_t* im = reinterpret_cast<uint16_t*>(smem);
  constexpr int RS = kPPEpiRow16;
  bar();
#pragma unroll
  for (int bh = 0; bh < 2; ++bh)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = bh * 128 + bc + j * 16 + 4 * (lane >> 4);
      float bq[4] = {0.f, 0.f, 0.f, 0.f};
      bias4(n0 + col, bq);
#pragma unroll
      for (int ah = 0; ah < 2; ++ah)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = ah * 128 + ar + i * 16 + (lane & 15);
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = elem(acc[ah][i][bh][j][e] * alpha + bq[e]);
          *reinterpret_cast<uint2*>(im + r * RS + col) = make_uint2(pack(v[0], v[1]), pack(v[2], v[3]));
        }
    }
  bar();
  const int ecb = (tid & 31) * 8, erb = tid >> 5;
  const int nb = n0 + ecb;
  if (nb < N) {
#pragma unroll 4
    for (int step = 0; step < 16; ++step) {
      const int r = step * 16 + erb;
      const int m = m0 + r;
      if (m >= M) break;
      *reinterpret_cast<uint4*>(c + (int64_t)m * ldc + nb) = *reinterpret_cast<const uint4*>(im + r * RS + ecb);
    }
  }
}

}  // namespace pa
