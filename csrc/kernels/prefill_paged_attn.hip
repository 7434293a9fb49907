// Paged prefill attention for gfx950: a chunk of new query tokens per sequence over the paged KV cache (bf16 or
// int8 storage), the chunk's own K / V already in the cache. Chunked prefill, prefix-cache prefill and
// speculative verify: more than one token per sequence at a per-sequence start position.
//
// Semantics: q [T, H, 128] packed by cu_q [B + 1]; ctx_lens[b] = cache positions the last chunk token of sequence
// b sees. With n_b = cu_q[b+1] - cu_q[b] and start_b = max(ctx_lens[b] - n_b, 0), chunk token i attends to cache
// positions 0 .. start_b + i (causal, bottom-right aligned, per sequence). Key t of kv head hk sits at
// tables[b, t / bs] * blk_stride + hk * head_stride + (t % bs) * 128, the addressing of decode_attn.hip.
//
// Work split: one workgroup (4 waves) per (query tile, kv head, sequence). A query tile is 128 MFMA columns:
// 128 / G consecutive chunk tokens x the G = H / Hkv heads of the GQA group (column c = token * G + head), so the
// group shares every K / V tile as the decode kernel's group does. Each wave owns 32 columns, each lane one
// column; its causal limit is start_b + token. All lengths are read on the device: the grid's tile count comes
// from a host bound on n_b, and workgroups past a sequence's last tile exit uniformly.
//
// Data movement and math are fa_fwd_kernel's (flash_attn_kernels.h): Q fragments in registers; K / V in 64-key
// tiles through two LDS stages in the img_off image; S^T = K Q^T with v_mfma_f32_32x32x16_bf16 so the softmax is
// in-lane; V^T by ds_read_b64_tr_b16; exp2-domain online softmax with the scale folded in and the deferred
// rescale; P rounded to bf16 for the PV MFMA; O normalised and written once. What differs:
//   * the block-table gather is in the per-lane source address of the LDS-DMA: each lane looks its key row up in
//     `tables`. The key index is clamped to ctx_lens[b] - 1 before the lookup, so a tile row past the context
//     re-reads a valid key (masked to -inf): never-written slots and spare table entries are never read (a NaN
//     there would poison the row through 0 * NaN in the PV product);
//   * a wave skips the math of tiles beyond its own last row's limit (it still stages and meets the barrier);
//   * uint8 caches (int8 + 128): LDS-DMA cannot convert, so a key row is loaded as bytes into registers one tile
//     ahead, u - 128 converted to bf16 (exact, |value| <= 128) and written into the same image with ds_write.
//     k_dq[hk] multiplies the exp2 constant, v_dq[hk] the normalised O; both are read from device memory.
// No split over the keys.
#include "flash_attn_kernels.h"

namespace {

struct PrefillArgs {
  const uint16_t* q;      // [T, H, 128]
  const void* kc;         // [nb, Hkv, bs, 128] (strides below)
  const void* vc;
  const float* k_dq;      // [Hkv], uint8 caches only
  const float* v_dq;
  const int* tables;      // [B, max_blocks]
  const int* cu_q;        // [B + 1]
  const int* ctx_lens;    // [B]
  uint16_t* out;          // [T, H, 128]
  int H, lg;              // lg = log2(G)
  int bs, max_blocks;
  int64_t blk_stride, head_stride;  // in elements
  float scale_log2;
};

// 8 cache bytes -> 8 bf16 of u - 128 (the fp32 value is an integer of at most 8 bits: its top half is the bf16)
__device__ __forceinline__ uint4 q8_to_bf16(uint2 v) {
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t x = j < 2 ? v.x : v.y;
    const int s = (j & 1) * 16;
    const float lo = (float)((x >> s) & 0xffu) - 128.f;
    const float hi = (float)((x >> (s + 8)) & 0xffu) - 128.f;
    w[j] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// CT: cache storage, uint16_t (bf16 bits) or uint8_t (int8 + 128)
template <typename CT>
__global__ __launch_bounds__(256, 2) void paged_prefill_k(PrefillArgs p) {
  constexpr bool Q8 = sizeof(CT) == 1;
  constexpr int D = 128, NCH = D / 8, KS = D / 16, NDT = D / 32, BN = 64;
  constexpr int TILE_BYTES = BN * D * 2;
  constexpr int NI = TILE_BYTES / 1024 / 4;  // glds per wave per tensor per tile
  constexpr float kDefer = 8.f;
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE_BYTES];

  const int b = blockIdx.z, hk = blockIdx.y;
  const int tpt = 128 >> p.lg;  // tokens per tile
  const int q_start = p.cu_q[b];
  const int n_b = p.cu_q[b + 1] - q_start;
  const int qt = (int)(gridDim.x - 1 - blockIdx.x);  // the heaviest tiles first
  if (qt * tpt >= n_b) return;                       // uniform: also n_b = 0
  const int ctx = p.ctx_lens[b];
  const int start = max(ctx - n_b, 0);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, hf = lane >> 5;
  const int col = w * 32 + r;
  const int tok = qt * tpt + (col >> p.lg);
  const int h = (hk << p.lg) + (col & ((1 << p.lg) - 1));
  const bool row_ok = tok < n_b;
  const int lim = start + tok;  // last visible cache position of this lane's row

  float c = p.scale_log2, vdq = 1.f;
  if constexpr (Q8) {
    c *= p.k_dq[hk];
    vdq = p.v_dq[hk];
  }

  Frag qf[KS];
  {
    const uint16_t* qrow = p.q + ((int64_t)(q_start + (row_ok ? tok : 0)) * p.H + h) * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (row_ok) qf[ks].u = *reinterpret_cast<const uint4*>(qrow + ks * 16 + hf * 8);
      else qf[ks].u = make_uint4(0, 0, 0, 0);
    }
  }

  f32x16 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  const int tok_last = min(qt * tpt + tpt, n_b) - 1;
  const int kv_end = min(ctx, start + tok_last + 1);
  const int n_tiles = kv_end > 0 ? (kv_end + BN - 1) / BN : 0;
  // this wave's rows: first / last visible position (rows past n_b are never written)
  const int wave_lo = start + qt * tpt + ((w * 32) >> p.lg);
  const int wave_hi = start + qt * tpt + ((w * 32 + 31) >> p.lg);
  const bool wave_live = qt * tpt + ((w * 32) >> p.lg) < n_b;  // a wave wholly past the chunk only stages

  // element offset of cache row `key` of this (sequence, kv head); the key is clamped into the context and the
  // block index into the table row
  const int* trow = p.tables + (int64_t)b * p.max_blocks;
  const int64_t hoff = (int64_t)hk * p.head_stride;
  auto row_off = [&](int key) -> int64_t {
    key = key < ctx ? key : ctx - 1;
    const int blk = key / p.bs;
    const int slot = key - blk * p.bs;
    return (int64_t)trow[min(blk, p.max_blocks - 1)] * p.blk_stride + hoff + (int64_t)slot * D;
  };

  // bf16 cache: LDS-DMA of tile `tile` into stage `stage` (lane-linear LDS writes; the swizzle is in the source chunk)
  auto issue = [&](int tile, int stage) {
    const char* kdst = smem + stage * 2 * TILE_BYTES;
    const char* vdst = kdst + TILE_BYTES;
    const uint16_t* kc = reinterpret_cast<const uint16_t*>(p.kc);
    const uint16_t* vc = reinterpret_cast<const uint16_t*>(p.vc);
    int64_t off[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {  // the table lookups first: their wait retires nothing but themselves
      const int qq = w * NI + i;
      const int row = qq * 4 + (lane >> 4), slot = lane & 15;
      const int ch = (img_off<NCH>(row, slot) - row * (NCH * 16)) / 16;  // slot ^ swizzle(row)
      off[i] = row_off(tile * BN + row) + ch * 8;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int qq = w * NI + i;
      glds16(kc + off[i], kdst + qq * 1024);
      glds16(vc + off[i], vdst + qq * 1024);
    }
  };

  // uint8 cache: 64 rows x 128 bytes per tensor = 2 x 16 bytes per thread, loaded a tile ahead into registers,
  // converted and written to the image after the current tile's math
  uint4 kreg[2], vreg[2];
  auto q8_load = [&](int tile) {
    const uint8_t* kc = reinterpret_cast<const uint8_t*>(p.kc);
    const uint8_t* vc = reinterpret_cast<const uint8_t*>(p.vc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = tid + 256 * i;  // piece: row pc / 8, bytes 16 (pc % 8) ..
      const int64_t off = row_off(tile * BN + (pc >> 3)) + (pc & 7) * 16;
      kreg[i] = *reinterpret_cast<const uint4*>(kc + off);
      vreg[i] = *reinterpret_cast<const uint4*>(vc + off);
    }
  };
  auto q8_store = [&](int stage) {
    char* kdst = smem + stage * 2 * TILE_BYTES;
    char* vdst = kdst + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = tid + 256 * i;
      const int row = pc >> 3, ch = 2 * (pc & 7);
      const int o0 = img_off<NCH>(row, ch), o1 = img_off<NCH>(row, ch + 1);
      *reinterpret_cast<uint4*>(kdst + o0) = q8_to_bf16(make_uint2(kreg[i].x, kreg[i].y));
      *reinterpret_cast<uint4*>(kdst + o1) = q8_to_bf16(make_uint2(kreg[i].z, kreg[i].w));
      *reinterpret_cast<uint4*>(vdst + o0) = q8_to_bf16(make_uint2(vreg[i].x, vreg[i].y));
      *reinterpret_cast<uint4*>(vdst + o1) = q8_to_bf16(make_uint2(vreg[i].z, vreg[i].w));
    }
  };

  const int gi = lane & 15, qq4 = gi >> 2, pp = gi & 3, G1 = (lane >> 4) & 1;
  if (n_tiles > 0) {
    if constexpr (Q8) {
      q8_load(0);
      q8_store(0);
    } else {
      issue(0, 0);
    }
  }
  for (int t = 0; t < n_tiles; ++t) {
    const bool more = t + 1 < n_tiles;
    if constexpr (Q8) {
      __syncthreads();  // tile t is in LDS (everyone's ds_write), stage (t+1)&1 is free
      if (more) q8_load(t + 1);
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of tile t are in LDS
      bar();                                             // ... everyone's, and stage (t+1)&1 is free
      if (more) issue(t + 1, (t + 1) & 1);
    }
    const char* ks_lds = smem + (t & 1) * 2 * TILE_BYTES;
    const char* vs_lds = ks_lds + TILE_BYTES;
    const int kv0 = t * BN;

    if (wave_live && kv0 <= wave_hi) {  // wave-uniform: a tile past the wave's last row is masked for all its rows
      f32x16 sacc[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        sacc[kt] = zero16();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          Frag a;
          a.u = lds_b128(ks_lds, img_off<NCH>(kt * 32 + r, 2 * ks + hf));
          sacc[kt] = mfma32<false>(a, qf[ks], sacc[kt]);
        }
      }
      if (kv0 + BN > ctx || kv0 + BN - 1 > wave_lo) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int kj = kv0 + kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * hf;
            if (kj >= ctx || kj > lim) sacc[kt][i] = -INFINITY;
          }
      }
      float mloc = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) mloc = fmaxf(mloc, sacc[kt][i]);
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
      const float m_new = fmaxf(m_run, mloc);
      // (m_new - m_run) * c: +inf on a row's first live tile, NaN while the row is all -inf (no rescale)
      if (__ballot((m_new - m_run) * c > kDefer)) {
        const float alpha = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m_run - m_new) * c);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
      }
      const float mc = (m_run == -INFINITY) ? 0.f : m_run * c;
      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kt][i], c, -mc));
          sacc[kt][i] = e;
          psum += e;
        }
      l_run += psum;

      Frag pf[2][2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float tmp[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) tmp[j] = sacc[kt][8 * s + j];
          pf[kt][s] = pack8<false>(tmp);
        }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int cch = (dt * 32 + 16 * G1) / 8 + (pp >> 1);
        const int cb = 8 * (pp & 1);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int R0 = kt * 32 + 16 * s + 4 * hf;
            Frag a;
            a.h[0] = lds_tr(vs_lds + (img_off<NCH>(R0 + qq4, cch) + cb));
            a.h[1] = lds_tr(vs_lds + (img_off<NCH>(R0 + 8 + qq4, cch) + cb));
            oacc[dt] = mfma32<false>(a, pf[kt][s], oacc[dt]);
          }
        }
      }
    }
    if constexpr (Q8) {
      if (more) q8_store((t + 1) & 1);
    }
  }

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? vdq / l_tot : 0.f;
  if (row_ok) {
    uint16_t* orow = p.out + ((int64_t)(q_start + tok) * p.H + h) * D;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = dt * 32 + 8 * g + 4 * hf;
        uint2 v2;
        v2.x = pack_bf16(oacc[dt][4 * g + 0] * inv, oacc[dt][4 * g + 1] * inv);
        v2.y = pack_bf16(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
        *reinterpret_cast<uint2*>(orow + d0) = v2;
      }
    }
  }
}

template <typename CT>
int launch_prefill(const void* q, const void* kc, const void* vc, const float* k_dq, const float* v_dq,
                   const int* tables, const int* cu_q, const int* ctx_lens, void* out, int B, int H, int Hkv, int D,
                   int bs, int max_blocks, int max_q, int64_t blk_stride, int64_t head_stride, float scale,
                   hipStream_t st) {
  if (D != 128 || Hkv < 1 || H % Hkv != 0 || bs < 1 || max_blocks < 1) return 3;
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return 4;
  // 16-byte row pieces: strides in elements of CT
  const int align = 16 / (int)sizeof(CT);
  if (blk_stride % align != 0 || head_stride % align != 0) return 6;
  if (B < 0 || B > 65535 || Hkv > 65535) return 7;
  if (B == 0 || max_q <= 0) return 0;
  PrefillArgs a;
  a.q = (const uint16_t*)q; a.kc = kc; a.vc = vc; a.k_dq = k_dq; a.v_dq = v_dq;
  a.tables = tables; a.cu_q = cu_q; a.ctx_lens = ctx_lens; a.out = (uint16_t*)out;
  a.H = H; a.lg = G == 1 ? 0 : (G == 2 ? 1 : (G == 4 ? 2 : 3));
  a.bs = bs; a.max_blocks = max_blocks; a.blk_stride = blk_stride; a.head_stride = head_stride;
  a.scale_log2 = scale * kLog2e;
  const int tpt = 128 / G;
  dim3 grid((unsigned)((max_q + tpt - 1) / tpt), (unsigned)Hkv, (unsigned)B);
  hipLaunchKernelGGL(paged_prefill_k<CT>, grid, dim3(256), 0, st, a);
  PA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// q / out [T, H, 128] bf16, the step's tokens packed per sequence by cu_q [B + 1] int32; ctx_lens [B] int32: cache
// positions the last chunk token sees (the chunk is in the cache); caches bf16 addressed as in pa_paged_decode_attn;
// tables [B, max_blocks] int32. max_q: host upper bound on the tokens of one sequence (sizes the grid). Rows of
// `out` that cu_q does not cover are not written.
PA_EXPORT int pa_paged_prefill_attn(const void* q, const void* kc, const void* vc, const int* tables, const int* cu_q,
                                    const int* ctx_lens, void* out, int B, int H, int Hkv, int D, int bs,
                                    int max_blocks, int max_q, int64_t blk_stride, int64_t head_stride, float scale,
                                    hipStream_t st) {
  return launch_prefill<uint16_t>(q, kc, vc, nullptr, nullptr, tables, cu_q, ctx_lens, out, B, H, Hkv, D, bs,
                                  max_blocks, max_q, blk_stride, head_stride, scale, st);
}

// The same over uint8 caches (int8 value + 128): a cached element is (u - 128) * k_dq[kv head] (v_dq for V), the
// [Hkv] fp32 scales read on the device. The chunk's own tokens are read back quantised. Strides in elements (= bytes).
PA_EXPORT int pa_paged_prefill_attn_q8(const void* q, const void* kc, const void* vc, const float* k_dq,
                                       const float* v_dq, const int* tables, const int* cu_q, const int* ctx_lens,
                                       void* out, int B, int H, int Hkv, int D, int bs, int max_blocks, int max_q,
                                       int64_t blk_stride, int64_t head_stride, float scale, hipStream_t st) {
  if (k_dq == nullptr || v_dq == nullptr) return 5;
  return launch_prefill<uint8_t>(q, kc, vc, k_dq, v_dq, tables, cu_q, ctx_lens, out, B, H, Hkv, D, bs, max_blocks,
                                 max_q, blk_stride, head_stride, scale, st);
}
