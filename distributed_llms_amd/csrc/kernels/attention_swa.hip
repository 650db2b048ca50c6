// Sliding-window paged attention (Mistral): a query at position p attends to the keys max(0, p - W + 1) .. p.
// Same cache as attention.hip -- 32-token blocks, K rows in krow32 order, V^T in groups of 8 -- and the same
// 16x16x32 MFMA chunk code (attention_common.h), with the window's lower bound masked where it can fall.
// Both kernels read a rotated q (after rope_cache_append) and walk only the blocks a window touches, so
// their time follows min(ctx, W) and their block ids are addressed from the window's first block on:
// neither depends on how wide the block table is.
#include <type_traits>

#include "attention_common.h"
#include "launch_host.h"
#include "launchers.h"

namespace dllm {

// ---------------------------------------------------------------------------
// Windowed decode: grid (num_splits, Hkv / WPB, B), one wave per (split, kv head, sequence), as
// attn_decode_kernel.  The splits are WINDOW-RELATIVE: the span of a sequence of ctx keys starts at
// block sb = max(0, ctx - W) / 32 and ends with block (ctx - 1) / 32, at most ceil(W / 32) + 1 blocks,
// and split s walks the blocks [sb + s * split_blocks, sb + (s + 1) * split_blocks) of it.  The host
// picks (num_splits, split_blocks) from the batch bucket and W alone (ops.decode_window_plan), so the
// grid knows nothing of the real context or the table width, no split of a long context is empty, and a
// sequence's keys are partitioned -- and its partials summed -- the same way whatever it is batched with.
// Blocks before sb are never loaded; the lower bound can only cut block sb and the length only the last
// block, but both compares run in every chunk: the wave is bound by the KV stream, and one instruction
// stream keeps the depth-2 load pipeline of the causal kernel intact.
// ---------------------------------------------------------------------------
template <int D, int WPB>
__global__ void __launch_bounds__(WPB * 64, 2) attn_decode_win_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ q, const bf16* __restrict__ k_cache,
    const bf16* __restrict__ v_cache, const int32_t* __restrict__ block_tables,
    const int32_t* __restrict__ seq_lens, float* __restrict__ part_o, float* __restrict__ part_ml, int hq, int hkv,
    int max_blocks, int split_blocks, int window, float scale_log2) {
  const int split = blockIdx.x, b = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int kvh = blockIdx.y * WPB + (threadIdx.x >> 6);
  const int nsplit = gridDim.x;
  const int G = hq / hkv;
  const int r = lane & 15, g = lane >> 4;
  // a length the table cannot hold is cut to it: no block id is read past the row
  const int ctx = max(0, min(seq_lens[b], max_blocks * kBS));
  const int lo = max(0, ctx - window);              // first admissible key
  const int eb = (ctx + kBS - 1) / kBS;             // blocks of the context (exclusive end of the span)
  const int c0 = min(lo / kBS + split * split_blocks, eb);
  const int c1 = min(c0 + split_blocks, eb);
  const int32_t* bt = block_tables + (size_t)b * max_blocks;
  const int blk_first = lane < min(64, c1 - c0) ? bt[c0 + lane] : 0;

  // Q^T fragments: column r = head kvh * G + r (zero beyond G)
  bf16x8 qf[D / 32];
  const bool col_ok = r < G;
  const bf16* qrow = q + ((size_t)b * hq + kvh * G + (col_ok ? r : 0)) * D;
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(qrow + ks * 32 + 8 * g);
    if (!col_ok) v = bf16x8{};
    qf[ks] = v;
  }
  WaveState<D> st;
  init_state(st);
  const int kmax = ctx - 1;
  const size_t kv_head_stride = (size_t)kBS * D;
  // the context's last block holds nadm keys: load only the rows and V^T groups that hold them
  // (load_chunk_rows), as the causal decode does
  const int ctail = eb - 1;
  const int nadm = ctx - ctail * kBS;
  const int na_t = 4 * (nadm >> 3) + min(nadm & 7, 4), nb_t = 4 * (nadm >> 3) + max((nadm & 7) - 4, 0);
  const int ng_t = (nadm + 7) >> 3;
  const int kvh_u = __builtin_amdgcn_readfirstlane(kvh);
  auto load = [&](KVChunk<D>& c, int chunk, int blk) {
    const size_t base = ((size_t)blk * hkv + kvh_u) * kv_head_stride;
    const bool tail = chunk == ctail;
    load_chunk_rows<D>(c, k_cache + base, v_cache + base, __builtin_amdgcn_readfirstlane(tail ? na_t : 16),
                       __builtin_amdgcn_readfirstlane(tail ? nb_t : 16),
                       __builtin_amdgcn_readfirstlane(tail ? ng_t : 4), lane);
  };
  for (int cb = c0; cb < c1; cb += 64) {            // 64 chunks (2048 keys) of block ids per pass
    const int n = min(64, c1 - cb);
    const int my_blk = cb == c0 ? blk_first : (lane < n ? bt[cb + lane] : 0);
    KVChunk<D> cur, nxt;
    load(cur, cb, __builtin_amdgcn_readlane(my_blk, 0));
    int j = 0;
    for (; j + 2 <= n; j += 2) {                    // ping-pong: cur <-> nxt
      load(nxt, cb + j + 1, __builtin_amdgcn_readlane(my_blk, j + 1));
      compute_chunk<D, true, true>(st, qf, cur, (cb + j) * kBS, kmax, scale_log2, lane, lo);
      if (j + 2 < n) load(cur, cb + j + 2, __builtin_amdgcn_readlane(my_blk, j + 2));
      compute_chunk<D, true, true>(st, qf, nxt, (cb + j + 1) * kBS, kmax, scale_log2, lane, lo);
    }
    if (j < n) compute_chunk<D, true, true>(st, qf, cur, (cb + j) * kBS, kmax, scale_log2, lane, lo);
  }
  float lt = st.lsum;
  lt = rows_sum(lt);
  if (!col_ok) return;                              // after the last MFMA: divergence is safe
  const int h = kvh * G + r;
  if (nsplit == 1) {
    bf16* orow = out + ((size_t)b * hq + h) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = f2bf(lt > 0.f ? st.acc[dt][i] / lt : 0.f);
      *reinterpret_cast<bf16x4*>(orow + dt * 16 + 4 * g) = o;
    }
  } else {
    // every split writes its partial, an empty one (a context shorter than the window) o = 0, m = -inf,
    // l = 0: attn_split_reduce_kernel sums them in split order and reads nothing it did not get
    const size_t pi = ((size_t)b * hq + h) * nsplit + split;
    float* po = part_o + pi * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<f32x4*>(po + dt * 16 + 4 * g) = st.acc[dt];
    if (g == 0) { part_ml[pi * 2] = st.m; part_ml[pi * 2 + 1] = lt; }
  }
}

// ---------------------------------------------------------------------------
// Windowed prefill: the LDS-shared kernel (attn_prefill_lds_kernel, version 4) with a windowed walk.  A
// workgroup owns kWaves x NT column tiles (kWaves * NT * 16/G query rows x G heads) of one (sequence, kv
// head) and streams K / V chunks once through the 3-deep LDS-DMA ring -- but only the chunks from the
// one the window of its EARLIEST row touches to its diagonal chunk, and it stages only those block ids
// (at most (W + rows - 2) / 32 + 2 of them), addressed from the walk's first chunk: the table may be any
// width.  Per wave and chunk, wave-uniform: a chunk that lies wholly inside every column's window and
// below every column's diagonal runs unmasked; one that begins before the lower bound of the wave's last
// row, or reaches past the diagonal of its first, takes both compares; one outside all of the wave's
// windows is skipped.
// ---------------------------------------------------------------------------
constexpr int kWinMaxIds = 1024;   // block ids a workgroup stages: 4 KiB beside the 48 KiB ring (D = 128)

template <int D, int G, int NT>
__global__ void __launch_bounds__(kWaves * 64, 2) attn_prefill_win_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ q, const bf16* __restrict__ k_cache,
    const bf16* __restrict__ v_cache, const int32_t* __restrict__ block_tables,
    const int32_t* __restrict__ cu_seqlens_q, const int32_t* __restrict__ seq_lens, int hq, int hkv,
    int max_blocks, int window, float scale_log2) {
  constexpr int WV = kWaves;
  constexpr int R = 16 / G;                       // query rows per column tile
  constexpr int CH = 2 * kBS * D;                 // bf16 elements per staged chunk (K block + V^T block)
  constexpr int NB = 3;                           // ring depth
  constexpr int GL = D / 8 / WV;                  // LDS-DMA wave-instructions per wave per chunk
  static_assert(GL >= 1 && GL * WV * 512 == CH, "chunk pieces");
  constexpr int SLOTS = 2 * D / 16;               // 16-B slots per K row
  constexpr int ROWS_PER_I = 1024 / (2 * D);      // K rows per 1 KiB wave-instruction
  __shared__ __attribute__((aligned(16))) bf16 smem[NB * CH + 2 * kWinMaxIds];
  int* ids = reinterpret_cast<int*>(smem + NB * CH);

  int qt, kvh, b;
  xcd_order(qt, kvh, b);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int qs = cu_seqlens_q[b], ql = cu_seqlens_q[b + 1] - qs;
  const int wg_row0 = qt * WV * R * NT;
  if (wg_row0 >= ql) return;                      // workgroup-uniform
  const int row0 = wg_row0 + w * R * NT;
  const bool active = row0 < ql;                  // wave-uniform; inactive waves still stage
  const int ctx = seq_lens[b];
  const int qpos0 = ctx - ql;
  bf16x8 qf[NT][D / 32];
  int kmax_col[NT], kmin_col[NT];
  WaveState<D> st[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int crow = row0 + t * R + r / G, ch = r % G;
    const bool ok = crow < ql;
    kmax_col[t] = ok ? qpos0 + crow : -1;
    kmin_col[t] = max(0, kmax_col[t] - window + 1);
    const bf16* qrow = q + ((size_t)(qs + (ok ? crow : 0)) * hq + kvh * G + ch) * D;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(qrow + ks * 32 + 8 * g);
      if (!ok) v = bf16x8{};
      qf[t][ks] = v;
    }
    init_state(st[t]);
  }
  // the workgroup's walk: from the chunk of its first row's lower bound to its last row's diagonal chunk
  // (a sequence the table cannot hold is cut to the table: no block id is read past the row)
  const int wg_kmax = qpos0 + min(wg_row0 + WV * R * NT, ql) - 1;
  const int cbeg = max(0, qpos0 + wg_row0 - window + 1) / kBS;
  const int nch = min(min(wg_kmax / kBS + 1, max_blocks) - cbeg, kWinMaxIds);
  // the wave's own bounds (wave-uniform).  wave_kmin: the smallest diagonal over its columns, -1 when any
  // of its rows is past the sequence (those columns take the masked path to stay exactly zero);
  // wave_lo_min / wave_lo_max: the lower bounds of its first and its last row
  const int wave_kmax = active ? qpos0 + min(row0 + R * NT, ql) - 1 : -1;
  const int wave_kmin = row0 + R * NT <= ql ? qpos0 + row0 : -1;
  const int wave_lo_min = max(0, qpos0 + row0 - window + 1);
  const int wave_lo_max = max(0, wave_kmax - window + 1);
  const int32_t* bt = block_tables + (size_t)b * max_blocks;
  for (int i = threadIdx.x; i < nch; i += WV * 64) ids[i] = bt[cbeg + i];
  // retire the q and block-id loads before the first LDS-DMA: their uses inside the loop
  // would otherwise make hipcc wait vmcnt(0) there, draining the ring every chunk
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) asm volatile("" ::"v"(qf[t][ks]));
  __syncthreads();

  const size_t kv_head_stride = (size_t)kBS * D;
  const size_t head_off = (size_t)kvh * kv_head_stride;
  const size_t blk_stride = (size_t)hkv * kv_head_stride;
  // wave w issues 1 KiB pieces w*GL .. w*GL+GL-1 of walked chunk i (pieces 0..D/16-1: K, the rest: V^T)
  auto stage = [&](int i_chunk, int buf) {
    const size_t base = (size_t)ids[i_chunk] * blk_stride + head_off;
    bf16* dst = smem + buf * CH;
#pragma unroll
    for (int j = 0; j < GL; ++j) {
      const int i = w * GL + j;                   // 1 KiB piece of the 2 * 32 * D * 2 B chunk
      const bf16* src;
      if (i < D / 16) {                           // K block, swizzled slots
        const int rr = i * ROWS_PER_I + lane / SLOTS, cs = lane % SLOTS;
        src = k_cache + base + (size_t)rr * D + (cs ^ (rr & (SLOTS - 1))) * 8;
      } else {                                    // V^T block, linear
        src = v_cache + base + (size_t)(i - D / 16) * 512 + lane * 8;
      }
      __builtin_amdgcn_global_load_lds((glb_vptr_a)src, (lds_vptr_a)(dst + i * 512), 16, 0, 0);
    }
  };
  auto read = [&](KVChunk<D>& c, int buf) {
    const bf16* kb = smem + buf * CH;
    const bf16* vb = kb + kBS * D;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      const int cs = ks * 4 + g;
      c.ka[ks] = *reinterpret_cast<const bf16x8*>(kb + r * D + (cs ^ (r & (SLOTS - 1))) * 8);
      c.kb[ks] = *reinterpret_cast<const bf16x8*>(kb + (16 + r) * D + (cs ^ ((16 + r) & (SLOTS - 1))) * 8);
    }
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) c.v[dt] = *reinterpret_cast<const bf16x8*>(vb + g * 8 * D + (dt * 16 + r) * 8);
  };

  if (nch > 0) stage(0, 0);
  if (nch > 1) stage(1, 1);
  int buf = 0;
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) {
      if constexpr (GL == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else if constexpr (GL == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    KVChunk<D> kc;
    read(kc, buf);
    // buffer (c + 2) % NB was read in iteration c - 1, which every wave finished before the
    // barrier above (its fragments were consumed by MFMAs)
    if (c + 2 < nch) stage(c + 2, buf == 0 ? NB - 1 : buf - 1);
    const int k0 = (cbeg + c) * kBS;              // the chunk's first key
    if (k0 >= wave_lo_max && k0 + kBS - 1 <= wave_kmin) {    // inside every column's window: no mask
#pragma unroll
      for (int t = 0; t < NT; ++t) compute_chunk<D, false>(st[t], qf[t], kc, k0, kmax_col[t], scale_log2, lane);
    } else if (k0 <= wave_kmax && k0 + kBS - 1 >= wave_lo_min) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        compute_chunk<D, true, true>(st[t], qf[t], kc, k0, kmax_col[t], scale_log2, lane, kmin_col[t]);
    }
    buf = buf == NB - 1 ? 0 : buf + 1;
  }
  if (!active) return;
#pragma unroll
  for (int t = 0; t < NT; ++t) store_tile_direct<D, G>(out, st[t], row0 + t * R, qs, ql, hq, kvh, lane);
}

// ------------------------------------------------------------------ launchers
// Windowed decode: q [B, hq, D] rotated.  Split s of a sequence walks the blocks [s, s + 1) * split_blocks
// of its window's span; num_splits * split_blocks must cover ceil(window / 32) + 1 blocks.  part_o [B, hq,
// num_splits, D] and part_ml [B, hq, num_splits, 2] floats (num_splits > 1)
void paged_attention_decode_window(uintptr_t out, uintptr_t q, uintptr_t k_cache, uintptr_t v_cache,
                                   uintptr_t block_tables, uintptr_t seq_lens, uintptr_t part_o, uintptr_t part_ml,
                                   int batch, int hq, int hkv, int d, int block_size, int max_blocks, int window,
                                   int num_splits, int split_blocks, float scale, uintptr_t stream) {
  DLLM_HOST_CHECK(block_size == kBS, "paged attention requires block_size 32");
  DLLM_HOST_CHECK(hkv >= 1 && hq % hkv == 0 && hq / hkv <= 16, "GQA group size must be <= 16");
  DLLM_HOST_CHECK(d == 64 || d == 128, "head_dim must be 64 or 128");
  DLLM_HOST_CHECK(window >= 1 && max_blocks >= 1, "window >= 1");
  DLLM_HOST_CHECK(num_splits >= 1 && split_blocks >= 1 &&
                      (long)num_splits * split_blocks >= ((long)window + kBS - 1) / kBS + 1,
                  "the splits must cover the window's span");
  DLLM_HOST_CHECK(num_splits == 1 || (part_o && part_ml), "split workspace");
  if (batch == 0) return;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float sl2 = scale * 1.4426950408889634f;
  const int wpb = hkv % 4 == 0 ? 4 : hkv % 2 == 0 ? 2 : 1;
  const dim3 grid(num_splits, hkv / wpb, batch);
  dispatch_value<128, 64>(d, "head_dim must be 64 or 128", [&](auto dc) {
    dispatch_value<4, 2, 1>(wpb, "decode attention: waves per workgroup", [&](auto wc) {
      constexpr int D = decltype(dc)::value, W = decltype(wc)::value;
      hipLaunchKernelGGL((attn_decode_win_kernel<D, W>), grid, dim3(64 * W), 0, s, (bf16*)out, (const bf16*)q,
                         (const bf16*)k_cache, (const bf16*)v_cache, (const int32_t*)block_tables,
                         (const int32_t*)seq_lens, (float*)part_o, (float*)part_ml, hq, hkv, max_blocks, split_blocks,
                         window, sl2);
    });
  });
  DLLM_HIP_CHECK(hipGetLastError());
  if (num_splits > 1) {
    dispatch_value<128, 64>(d, "head_dim must be 64 or 128", [&](auto dc) {
      constexpr int D = decltype(dc)::value;
      hipLaunchKernelGGL(attn_split_reduce_kernel<D>, dim3((unsigned)batch * hq), dim3(D), 0, s, (bf16*)out,
                         (const float*)part_o, (const float*)part_ml, num_splits);
    });
    DLLM_HIP_CHECK(hipGetLastError());
  }
}

// rows of q one workgroup of the windowed prefill owns
int prefill_window_tile_rows(int group) { return kWaves * (16 / group) * 2; }
// the largest window whose walked block ids fit the kernel's LDS list
int prefill_window_max(int group) { return (kWinMaxIds - 2) * kBS - prefill_window_tile_rows(group) + 2; }

// Windowed prefill: q [T, hq, D] rotated, the context (q's rows are its last tokens) in the paged cache
void paged_attention_prefill_window(uintptr_t out, uintptr_t q, uintptr_t k_cache, uintptr_t v_cache,
                                    uintptr_t block_tables, uintptr_t cu_seqlens_q, uintptr_t seq_lens, int batch,
                                    int hq, int hkv, int d, int block_size, int max_blocks, int max_q_len, int window,
                                    float scale, uintptr_t stream) {
  DLLM_HOST_CHECK(block_size == kBS, "paged attention requires block_size 32");
  DLLM_HOST_CHECK(d == 64 || d == 128, "head_dim must be 64 or 128");
  DLLM_HOST_CHECK(hkv >= 1 && hq % hkv == 0, "Hq % Hkv");
  const int g = hq / hkv;
  DLLM_HOST_CHECK(g >= 1 && g <= 16 && 16 % g == 0, "prefill attention: GQA group must be 1,2,4,8,16");
  DLLM_HOST_CHECK(window >= 1 && window <= prefill_window_max(g) && max_blocks >= 1,
                  "windowed prefill attention: the window's block ids must fit the LDS list");
  if (batch == 0 || max_q_len == 0) return;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float sl2 = scale * 1.4426950408889634f;
  const int rows_per_wg = prefill_window_tile_rows(g);
  const dim3 grid((max_q_len + rows_per_wg - 1) / rows_per_wg, hkv, batch);
  dispatch_value<128, 64>(d, "head_dim must be 64 or 128", [&](auto dc) {
    dispatch_value<1, 2, 4, 8, 16>(g, "prefill attention: GQA group must be 1,2,4,8,16", [&](auto gc) {
      hipLaunchKernelGGL((attn_prefill_win_kernel<decltype(dc)::value, decltype(gc)::value, 2>), grid,
                         dim3(kWaves * 64), 0, s, (bf16*)out, (const bf16*)q, (const bf16*)k_cache,
                         (const bf16*)v_cache, (const int32_t*)block_tables, (const int32_t*)cu_seqlens_q,
                         (const int32_t*)seq_lens, hq, hkv, max_blocks, window, sl2);
    });
  });
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
