// Device code shared by the paged attention kernels (attention.hip, attention_swa.hip): the 32-key chunk in
// registers, its loaders, the online-softmax update on the 16x16x32 MFMA, the split reduce and the tile epilogue.
#pragma once
#include "common.h"

namespace dllm {

constexpr int kBS = 32;       // tokens per KV block (== keys per MFMA chunk)
constexpr int kWaves = 4;     // waves per workgroup
typedef __attribute__((address_space(3))) void* lds_vptr_a;
typedef __attribute__((address_space(1))) void* glb_vptr_a;

template <int D>
struct WaveState {
  f32x4 acc[D / 16];
  float m;      // running max (log2 domain) of this lane's column
  float lsum;   // lane-partial softmax denominator
};

// One 32-key chunk's operands, loaded into registers: K rows as two 16-key A tiles (physical
// rows, see krow32 in common.h), V^T as the A fragments of the P.V MFMA (keys 8g..8g+7 of
// lane group g: one 16-byte load from the [4][D][8] V^T block).
template <int D>
struct KVChunk {
  bf16x8 ka[D / 32], kb[D / 32];
  bf16x8 v[D / 16];
};

template <int D>
__device__ __forceinline__ void load_chunk(KVChunk<D>& c, const bf16* __restrict__ kblk,
                                           const bf16* __restrict__ vblk, int lane) {
  const int r = lane & 15, g = lane >> 4;
  // default cache policy: prefill re-reads a sequence's K/V for every q tile (the decode wave, which
  // reads each line once per step, loads nontemporal: load_chunk_rows)
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    c.ka[ks] = *reinterpret_cast<const bf16x8*>(kblk + r * D + ks * 32 + 8 * g);
    c.kb[ks] = *reinterpret_cast<const bf16x8*>(kblk + (16 + r) * D + ks * 32 + 8 * g);
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt)
    c.v[dt] = *reinterpret_cast<const bf16x8*>(vblk + g * 8 * D + (dt * 16 + r) * 8);
}

// load_chunk for the decode wave, as buffer loads through three descriptors that END behind the rows
// and groups to load: 16 ka rows, 16 kb rows and 4 V^T groups for every chunk but a split's last,
// whose block is admissible only up to its first nadm keys (the rest is stale cache that
// compute_chunk masks to -inf).  krow32 puts keys 8j..8j+3 in rows 4j.. of the ka tile and keys
// 8j+4..8j+7 in rows 4j.. of the kb tile, so the admissible rows of each tile are a prefix of it
// (na, nb rows) and the admissible V^T groups ([4][D][8]) a prefix of the block (ng): the range
// check hands every lane beyond them zeros without a memory request.  The counts are scalars
// picked per chunk, so nothing selects or branches per lane, every chunk issues the same
// 2 * D/32 + D/16 loads, and the vmcnt the consumer waits for stays exact (a separate loader for
// the last chunk behind a wave-uniform branch compiled to a block that drained vmcnt(0) first).
// A masked score is -inf and its probability an exact 0 whatever finite bytes K / V held, so the
// result is bit-identical to loading the stale rows.
//   khead / vhead : the (block, kv head) tile's address, wave-uniform to the compiler as well
//                   (a descriptor built from anything else is read back lane by lane in a
//                   waterfall loop around each load)
template <int D>
__device__ __forceinline__ void load_chunk_rows(KVChunk<D>& c, const bf16* khead, const bf16* vhead, int na, int nb,
                                                int ng, int lane) {
  const auto ra = __builtin_amdgcn_make_buffer_rsrc((void*)khead, (short)0, na * D * 2, 0x00020000);
  const auto rb = __builtin_amdgcn_make_buffer_rsrc((void*)(khead + 16 * D), (short)0, nb * D * 2, 0x00020000);
  const auto rv = __builtin_amdgcn_make_buffer_rsrc((void*)vhead, (short)0, ng * 8 * D * 2, 0x00020000);
  // The lane offsets are worked out HERE, behind an opaque copy of the lane id: computed from `lane`
  // itself every `offset + fragment constant` is loop-invariant, hoisted out of the chunk loop and
  // held across it in a register of its own (12 at D = 128, which spilled).  Kept in this block, the
  // constants fold into the loads' immediate offsets.
  int l = lane;
  asm volatile("" : "+v"(l));
  const int r = l & 15, g = l >> 4;
  const int ok = (r * D + 8 * g) * 2, ov = (g * 8 * D + r * 8) * 2;
  // aux 2: nontemporal.  The decode wave reads each K/V line once per step (cold, HBM): nontemporal
  // loads cut the attention alone 41.4 -> 35.3 us at B=256 / ctx 192 (profiles/attn_fused_ablation.md)
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    c.ka[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, ok + ks * 64, 0, 2));
    c.kb[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rb, ok + ks * 64, 0, 2));
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt)
    c.v[dt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, ov + dt * 256, 0, 2));
}

// Online-softmax update of the wave's 16 columns with one loaded chunk.
//   kmax_col : last admissible key index for this lane's column (causal / range), inclusive
//   MASK     : false when the caller knows every key of the chunk is admissible for every column
//              (prefill chunks strictly below the diagonal): no per-score compare / select
// VALU economy (long prefill is VALU-bound: ~330 VALU per 32 MFMAs, MFMA 25 % busy --
// profiles/round5_prefill_attn_valu.md): the running max is taken on the raw scores and scaled
// once (x -> x * scale is monotonic, so the max is the same number), the scale folds into the
// exponent's FMA, and exp2 is the bare v_exp_f32 (libm's exp2f adds a denormal-range fix-up of
// four instructions per call; results below 2^-126 of the row max flush to zero), and the
// accumulator rescale is skipped when no column's max moved.
//   LOW      : sliding window (attention_swa.hip): keys below kmin_col, the column's first admissible key,
//              are masked as well; a compile-time choice, so the causal kernels' code has no trace of it
template <int D, bool MASK = true, bool LOW = false>
__device__ __forceinline__ void compute_chunk(WaveState<D>& st, const bf16x8 (&qf)[D / 32], const KVChunk<D>& c,
                                              int t0, int kmax_col, float scale_log2, int lane, int kmin_col = 0) {
  const int g = lane >> 4;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c.ka[ks], qf[ks], s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c.kb[ks], qf[ks], s1, 0, 0, 0);
  }
  float p[8];
  float cm = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (MASK) {
      const int k0 = t0 + 8 * g + i, k1 = t0 + 8 * g + 4 + i;   // S^T rows 4g+i / 16+4g+i (krow32)
      if constexpr (LOW) {
        p[i] = (k0 <= kmax_col && k0 >= kmin_col) ? s0[i] : -INFINITY;
        p[4 + i] = (k1 <= kmax_col && k1 >= kmin_col) ? s1[i] : -INFINITY;
      } else {
        p[i] = (k0 <= kmax_col) ? s0[i] : -INFINITY;
        p[4 + i] = (k1 <= kmax_col) ? s1[i] : -INFINITY;
      }
    } else {
      p[i] = s0[i];
      p[4 + i] = s1[i];
    }
    cm = fmaxf(cm, fmaxf(p[i], p[4 + i]));
  }
  cm = rows_max(cm);                                // VALU row swaps, no LDS round trip
  cm *= scale_log2;
  // No early exit here: MFMA reads all 64 lanes' operands regardless of EXEC, so every
  // lane must run the same instruction stream. A fully masked column uses mref = 0,
  // which turns its probabilities (and its alpha) into exact zeros.
  const float mn = fmaxf(st.m, cm);
  const float mref = (mn == -INFINITY) ? 0.f : mn;
  const float alpha = __builtin_amdgcn_exp2f(st.m - mref);
  st.m = mn;
  // exponent arguments two per v_pk_fma_f32 (the same fused multiply-add per element), the
  // probabilities summed as a pairwise tree on v_pk_add_f32: 4 + 4 VALU where scalar code takes 8 + 8
  bf16x8 pb;
  f32x2 e2[4];
  const f32x2 sc2 = {scale_log2, scale_log2}, mr2 = {-mref, -mref};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 x = __builtin_elementwise_fma(f32x2{p[2 * j], p[2 * j + 1]}, sc2, mr2);
    e2[j] = f32x2{__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
    pb[2 * j] = f2bf(e2[j][0]);
    pb[2 * j + 1] = f2bf(e2[j][1]);
  }
  const f32x2 s2 = (e2[0] + e2[1]) + (e2[2] + e2[3]);
  st.lsum = st.lsum * alpha + (s2[0] + s2[1]);
  // alpha is exactly 1 wherever the running max did not move (exp2(0)), the common case once a
  // row's max has settled: skip the accumulator rescale when that holds for the whole wave (bit-exact)
  if (__any(alpha != 1.f)) {
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) st.acc[dt] *= alpha;
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const bf16x8 va = c.v[dt];
    st.acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, st.acc[dt], 0, 0, 0);
  }
}

template <int D>
__device__ __forceinline__ void init_state(WaveState<D>& st) {
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) st.acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  st.m = -INFINITY;
  st.lsum = 0.f;
}

// out[bh, d] from the (o, m, l) partials of nsplit splits, summed in split order
template <int D>
__global__ void __launch_bounds__(D) attn_split_reduce_kernel(bf16* __restrict__ out,
                                                              const float* __restrict__ part_o,
                                                              const float* __restrict__ part_ml,
                                                              int nsplit) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const float* ml = part_ml + (size_t)bh * nsplit * 2;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ml[2 * s]);
  float num = 0.f, den = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float f = exp2f(ml[2 * s] - M);
      num += part_o[((size_t)bh * nsplit + s) * D + d] * f;
      den += ml[2 * s + 1] * f;
    }
  }
  out[(size_t)bh * D + d] = f2bf(den > 0.f ? num / den : 0.f);
}

// One 16-column tile's output straight from the accumulators (16/G query rows from trow0 x G heads):
// a lane holds 4 dims of one column per fragment, so a store instruction writes 32 bytes into each
// of 16 rows.  v3's epilogue, and v4's where its LDS output image does not fit.
template <int D, int G>
__device__ __forceinline__ void store_tile_direct(bf16* __restrict__ out, const WaveState<D>& st, int trow0, int qs,
                                                  int ql, int hq, int kvh, int lane) {
  const int r = lane & 15, g = lane >> 4;
  float lt = st.lsum;
  lt = rows_sum(lt);
  const int crow = trow0 + r / G, ch = r % G;
  if (crow < ql) {
    const float inv = lt > 0.f ? 1.f / lt : 0.f;
    bf16* orow = out + ((size_t)(qs + crow) * hq + kvh * G + ch) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = f2bf(st.acc[dt][i] * inv);
      *reinterpret_cast<bf16x4*>(orow + dt * 16 + 4 * g) = o;
    }
  }
}

// XCD-aware order: workgroups are dealt round-robin to the 8 XCDs in dispatch order, so the
// gridDim.x row tiles of one (sequence, kv head) -- which stream the same K / V chunks -- would
// land on gridDim.x different XCDs (each with its own L2).  Renumber so that they share one.
__device__ __forceinline__ void xcd_order(int& qt, int& kvh, int& b) {
  qt = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int nx = gridDim.x, ng = gridDim.y * gridDim.z;
  const int lin = blockIdx.x + nx * (blockIdx.y + gridDim.y * blockIdx.z);
  if (ng % 8 == 0) {
    const int xcd = lin & 7, slot = lin >> 3;            // slot-th workgroup of this XCD
    const int grp = (slot / nx) * 8 + xcd;
    qt = slot % nx;
    kvh = grp % gridDim.y;
    b = grp / gridDim.y;
  }
}

}  // namespace dllm
