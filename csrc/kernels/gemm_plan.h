// Host arithmetic shared by the tiled GEMM launchers (gemm.hip, gemm_fp8.hip): the balanced-tail plan of the
// 256 x 256 ping-pong kernels and the common operand check. Plain C++17 without HIP, so the planner that sizes the
// workspace (pa_gemm_pp_ws_bytes, pa_gemm_fp8_ws_bytes) is the one the launch uses, and tests/test_gemm_plan_host.py
// can compile it with the system compiler.
#pragma once
#include <climits>
#include <cstdint>

namespace pa {

// Tiles [full_tiles, tiles) are cut into `split` K slices whose fp32 256 x 256 partials go to a workspace of ws_bytes
// and are summed by a reduction launch of tiles - full_tiles blocks. split == 0: no tail, grid == tiles, ws_bytes == 0.
struct TailPlan {
  int tiles, full_tiles, split, grid;
  int64_t ws_bytes;
};

inline TailPlan make_tail_plan(int64_t tiles, int64_t full, int split) {
  const int64_t tail = split ? tiles - full : 0;
  return {(int)tiles, (int)(tiles - tail), split, (int)(tiles - tail + tail * split), tail * split * 65536 * 4};
}

inline int64_t tiles256(int64_t M, int64_t N) { return ((M + 255) / 256) * ((N + 255) / 256); }

// Tiles beyond the last whole wave of `cus` workgroups are split along K so the last wave has about one workgroup
// per CU. Only when the remainder covers at most half the chip and every slice keeps at least 4 K-tiles of k_tile.
inline TailPlan tail_plan(int64_t M, int64_t N, int64_t K, int k_tile, int cus) {
  const int64_t T = tiles256(M, N);
  const int64_t nk = K / k_tile;
  const int64_t r = T > cus ? T % cus : 0;
  if (r == 0 || 2 * r > cus) return make_tail_plan(T, T, 0);
  int sp = 1;
  while (r * sp * 2 <= cus && nk % (sp * 2) == 0 && nk / (sp * 2) >= 4) sp *= 2;
  return sp == 1 ? make_tail_plan(T, T, 0) : make_tail_plan(T, T - r, sp);
}

// Split-K over the same machinery: no whole tiles, every tile cut into `splits` slices.
inline TailPlan split_all_plan(int64_t M, int64_t N, int splits) { return make_tail_plan(tiles256(M, N), 0, splits); }

// The same product without its tail (no workspace was given).
inline TailPlan without_tail(const TailPlan& p) { return make_tail_plan(p.tiles, p.tiles, 0); }

// Requirements every bf16 tile kernel has on its operands: whole K tiles, 16-byte rows of A and B (lda, ldb in
// elements; M too when A is MN-major), 8-byte groups of C, and sizes the kernels' int fields can hold.
inline bool gemm_operands_ok(int64_t M, int64_t N, int64_t K, int k_tile, int64_t lda, int64_t ldb, int64_t ldc,
                             bool a_kmajor) {
  if (M > INT_MAX || N > INT_MAX || K > INT_MAX) return false;
  if (K % k_tile != 0 || N % 8 != 0 || lda % 8 != 0 || ldb % 8 != 0 || ldc % 4 != 0) return false;
  return a_kmajor || M % 8 == 0;
}

}  // namespace pa
