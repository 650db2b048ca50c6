// Fused LM head + log-softmax + gather: lp[i] = log softmax(bf16(x_i . W^T))[targets[i]] without ever
// storing a logit (contract: ops/reference.py lm_head_logprobs).  Prompt scoring needs one float per
// prompt row; the [T, V] logits of a long prefill step (32768 x 128256 bf16 = 8.4 GB) would be written
// once and read once for it.
//
// Design:
//  * the main loop is gemm_pf's: 4 waves as 2 x 2 on a 256 x 256 tile, 64-deep K-tiles in a 2-slot LDS-DMA
//    ring, schedule 2's MFMA stream (gemm_pp_loop.h), weights nontemporal (each is read once per row tile);
//  * grid = row tiles x S vocabulary ranges (S from the host: about one workgroup per free CU).  A
//    workgroup walks the 256-column tiles of its range with the ring running across tile boundaries: the
//    last K-tiles of a tile stage the first of the next, which re-reads the same 256 x K activation tile
//    (L2) against the next 256 weight rows (HBM, once);
//  * per tile the accumulators are rounded to bf16 in registers.  acc[r][c] lane l holds row
//    16 r + (l & 15), columns 16 c + 4 (l >> 4) + v of the wave's 128 x 128 quarter: a lane reduces its 32
//    columns of a row, v_permlane16/32_swap combine the four 16-lane rows (rows_max), and the wave's running
//    maximum m of that row is the same in the four lanes that share it.  The sum of exp(l - m) stays a
//    lane-private partial (rescaled only when m moved) and meets its three partners once, at the end of the
//    range.  The lane whose fragment holds the row's target column keeps that logit.  No barrier and no
//    other wave is involved: the two waves that share a row keep separate triples (in wave-private LDS
//    columns above the ring between tiles: the K loop leaves no registers for them);
//  * weight rows past V (the ragged last tile) are staged from row V - 1 and their columns count as -inf;
//    activation rows past T are staged from row T - 1 and never written;
//  * at the end of the range every wave writes (m, l, target logit or -inf) per row to the workspace
//    [T, 2 S, 3]; lm_head_logprobs_reduce, one thread per row, merges the 2 S triples in index order.
//    No atomics anywhere: the same inputs give the same bits;
//  * a row with a negative target gets 0.0 from the reduce, which reads nothing of it; a row tile whose
//    targets are all negative returns before its first load.
#include "common.h"
#include "gemm_pp_loop.h"
#include "launch_host.h"
#include "launchers.h"

namespace dllm {

namespace {
constexpr float kNegInf = -__builtin_huge_valf();

// The running triples live in LDS above the ring, one dword column per lane (conflict-free, wave-private):
// beside 256 accumulators and four fragment sets the register file has no room for 24 more values that the
// K loop never touches.  Inline asm like the fragment reads, so hipcc neither counts them nor orders them
// against the LDS-DMA pieces in flight; lp_wait() is their one wait.
template <int OFF>
__device__ __forceinline__ float lp_ld(uint32_t addr) {
  float r;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}
template <int OFF>
__device__ __forceinline__ void lp_st(uint32_t addr, float v) {
  asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "v"(v), "i"(OFF) : "memory");
}
__device__ __forceinline__ void lp_wait(float& a, float& b, float& c) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c)::"memory");
}
}

__global__ void __launch_bounds__(256, 1) lm_head_logprobs_kernel(const bf16* __restrict__ X, const bf16* __restrict__ W,
                                                                  const int* __restrict__ targets,
                                                                  float* __restrict__ ws, int T, int V, int K, int S) {
  constexpr int NW = 4, NWN = 2, BM = 256, BN = 256, TM = 128, TN = BN / NWN;
  constexpr int RT = TM / 16, CT = TN / 16;            // 8 x 8 accumulators per wave
  constexpr int SLOT = (BM + BN) * PBK, NB = 2;        // 2 x 64 KiB ring
  constexpr int GA = BM * PBK * 2 / 1024 / NW, GB = BN * PBK * 2 / 1024 / NW, G = GA + GB;
  using KT = PfKtile<RT, CT, G, NB>;
  constexpr int NST = 3 * RT;                          // state dwords per lane: (m, l, target logit) x RT row groups
  __shared__ __attribute__((aligned(16))) bf16 smem[NB * SLOT + NST * 256 * 2];
  static_assert(sizeof(smem) + 1024 <= 160 * 1024, "LDS");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv / NWN, wn = wv % NWN;
  const int m_t = blockIdx.x / S, rng = blockIdx.x % S;
  const int m0 = m_t * BM;
  // a row tile nobody asks about: gone before its first load (uniform)
  if (!__syncthreads_or(m0 + tid < T && targets[m0 + tid] >= 0)) return;
  const int ntv = (V + BN - 1) / BN;                   // S <= ntv (host): every range holds a tile
  const int n_begin = (int)((long)rng * ntv / S), n_end = (int)((long)(rng + 1) * ntv / S);
  const int nt = K / PBK;

  // ---- staging side: K-tile s_kt of column tile s_n.  Per-lane row offsets: A fixed for the workgroup
  // (rows past T clamp to T - 1), B per column tile (rows past V clamp to V - 1); the K-tile goes through
  // the SGPR offset
  const __amdgpu_buffer_rsrc_t rsA =
      __builtin_amdgcn_make_buffer_rsrc((void*)X, (short)0, (int)(unsigned)((long)T * K * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)W, (short)0, (int)(unsigned)((long)V * K * 2), 0x00020000);
  uint32_t chunk_q[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) chunk_q[par] = (uint32_t)(pswz(8 * par + (lane >> 3), lane & 7) * 16);
  uint32_t offA[GA], offB[GB];
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int q = wv * GA + j, r = 8 * q + (lane >> 3);
    offA[j] = (uint32_t)min(m0 + r, T - 1) * (uint32_t)(K * 2) + chunk_q[q & 1];
  }
  int s_n = n_begin, s_kt = 0;
  auto set_stage = [&]() {
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int q = wv * GB + j, r = 8 * q + (lane >> 3);
      offB[j] = (uint32_t)min(s_n * BN + r, V - 1) * (uint32_t)(K * 2) + chunk_q[q & 1];
    }
  };
  auto piece = [&](int slot, int p) {
    bf16* base = smem + slot * SLOT;
    if (p < GA)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_vptr_p)(base + (wv * GA + p) * 512), 16, (int)offA[p],
                                               s_kt * PBK * 2, 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_vptr_p)(base + BM * PBK + (wv * GB + p - GA) * 512), 16,
                                               (int)offB[p - GA], s_kt * PBK * 2, 0, 2);
  };
  // next staging K-tile; past the range's last tile: its K-tile nt - 1 again (a DUMMY piece into a slot
  // nobody reads again, so every K-tile issues exactly G pieces: static vmcnt counts)
  auto advance = [&]() {
    if (++s_kt == nt) {
      if (s_n + 1 < n_end) {
        ++s_n;
        s_kt = 0;
        set_stage();
      } else {
        s_kt = nt - 1;
      }
    }
  };

  const uint32_t lds_base = (uint32_t)(size_t)(lds_vptr_p)smem;
  uint32_t lane_off[2];
#pragma unroll
  for (int kh = 0; kh < 2; ++kh)
    lane_off[kh] = (uint32_t)((lane & 15) * 128 + ((4 * kh + (lane >> 4)) ^ (((lane & 15) >> 1) & 7)) * 16);
  const uint32_t a_off = (uint32_t)(wm * TM * 128), b_off = (uint32_t)(BM * 128 + wn * TN * 128);

  // the wave's running triple of row wm TM + 16 r + (lane & 15): m the same in the row's four lanes,
  // l this lane's share of the sum, tl the target's logit if one of this lane's columns is the target;
  // dword 3 r + {0, 1, 2} of this lane's state column
  const int lr = lane & 15, lq = lane >> 4;
  const uint32_t st = lds_base + (uint32_t)(NB * SLOT * 2) + (uint32_t)tid * 4;
  int tgt[RT];
  pp_static_for<RT>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    const int row = m0 + wm * TM + r * 16 + lr;
    lp_st<(3 * r) * 1024>(st, kNegInf);
    lp_st<(3 * r + 1) * 1024>(st, 0.f);
    lp_st<(3 * r + 2) * 1024>(st, kNegInf);
    tgt[r] = row < T ? targets[row] : -1;
  });

  f32x4 acc[RT][CT];
  bf16x8 fa0[RT], fb0[CT], fa1[RT], fb1[CT];

  // prologue: the first NB K-tiles in flight, K-tile 0 landed, its K-half 0 read
  set_stage();
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int p = 0; p < G; ++p) piece(j, p);
    advance();
  }
  pp_vm<(NB - 1) * G>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  KT::read_first(fa0, fb0, lds_base + lane_off[0], a_off, b_off);

  int slot = 0;
  for (int n_t = n_begin; n_t < n_end; ++n_t) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+a"(acc[i][j]));            // zeroed in place, in AGPRs
      }
    for (int t = 0; t < nt; ++t) {
      const int nslot = slot == NB - 1 ? 0 : slot + 1;
      const uint32_t base1 = lds_base + (uint32_t)(slot * SLOT * 2) + lane_off[1];
      const uint32_t base0 = lds_base + (uint32_t)(nslot * SLOT * 2) + lane_off[0];
      KT::run(acc, fa0, fb0, fa1, fb1, base0, base1, a_off, b_off, [&](int p) { piece(slot, p); });
      advance();
      slot = nslot;
    }
    // ---- the tile's logits, in registers only.  This lane's columns of row group r: col0 + 16 c + v
    const int col0 = n_t * BN + wn * TN + 4 * lq;
    const bool ragged = n_t * BN + BN > V;               // uniform: only the last tile masks columns
    pp_static_for<RT>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      // pin row r's accumulators in AGPRs up to here (as gemm_pf: no copy of all 256 at the loop's exit)
#pragma unroll
      for (int c = 0; c < CT; ++c) asm volatile("" : "+a"(acc[r][c]));
      float m = lp_ld<(3 * r) * 1024>(st), l = lp_ld<(3 * r + 1) * 1024>(st), tl = lp_ld<(3 * r + 2) * 1024>(st);
      float x[CT * 4];
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v) x[c * 4 + v] = bf2f(f2bf(acc[r][c][v]));
      if (ragged) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (col0 + 16 * c + v >= V) x[c * 4 + v] = kNegInf;
      }
      float mx = x[0];
#pragma unroll
      for (int i = 1; i < CT * 4; ++i) mx = fmaxf(mx, x[i]);
      mx = rows_max(mx);
      lp_wait(m, l, tl);
      if (mx > m) {                                      // the maximum moved: rescale this lane's share
        l *= __expf(m - mx);
        m = mx;
        lp_st<(3 * r) * 1024>(st, m);
      }
      // a wave whose columns so far are all past V has m = -inf and adds exp(-inf - 0) = 0
      const float ms = m == kNegInf ? 0.f : m;
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < CT * 4; ++i) sum += __expf(x[i] - ms);
      lp_st<(3 * r + 1) * 1024>(st, l + sum);
      const unsigned d = (unsigned)(tgt[r] - col0);      // the target's column relative to this lane's first
      if (d < (unsigned)TN && (d & 12) == 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (d == (unsigned)(16 * c + v)) tl = x[c * 4 + v];
        lp_st<(3 * r + 2) * 1024>(st, tl);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  // the dummy pieces of the last K-tiles must land before the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // ---- the wave's triples: partial kLmHeadWaves * rng + wn of row `row`
  const int np = kLmHeadWaves * S;
  pp_static_for<RT>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    float m = lp_ld<(3 * r) * 1024>(st), l = lp_ld<(3 * r + 1) * 1024>(st), tl = lp_ld<(3 * r + 2) * 1024>(st);
    lp_wait(m, l, tl);
    const float lsum = rows_sum(l), tsel = rows_max(tl);
    const int row = m0 + wm * TM + r * 16 + lr;
    if (lq == 0 && row < T) {
      float* p = ws + ((size_t)row * np + kLmHeadWaves * rng + wn) * 3;
      p[0] = m;
      p[1] = lsum;
      p[2] = tsel;
    }
  });
}

// one thread per row: lp = (t - M) - ln(sum_p l_p exp(m_p - M)), M = max_p m_p, over the row's np triples in
// index order; a negative target: 0.0, nothing read
__global__ void __launch_bounds__(256) lm_head_logprobs_reduce(float* __restrict__ out, const float* __restrict__ ws,
                                                               const int* __restrict__ targets, int T, int np) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= T) return;
  if (targets[row] < 0) {
    out[row] = 0.f;
    return;
  }
  const float* p = ws + (size_t)row * np * 3;
  float mx = kNegInf;
  for (int i = 0; i < np; ++i) mx = fmaxf(mx, p[3 * i]);
  float sum = 0.f, t = kNegInf;
  for (int i = 0; i < np; ++i) {
    const float mi = p[3 * i];
    if (mi > kNegInf) sum += p[3 * i + 1] * expf(mi - mx);
    t = fmaxf(t, p[3 * i + 2]);
  }
  out[row] = (t - mx) - logf(sum);
}

// out f32 [T]; x bf16 [T, K]; w bf16 [V, K]; targets i32 [T] (< 0: skip the row; < V checked by the caller);
// ws: f32 [T, kLmHeadWaves * S, 3]; S vocabulary ranges, 1 <= S <= ceil(V / 256)
void lm_head_logprobs(uintptr_t out, uintptr_t x, uintptr_t w, uintptr_t targets, uintptr_t ws, long ws_floats, int T,
                      int V, int K, int S, uintptr_t stream) {
  DLLM_HOST_CHECK(T >= 1 && V >= 1, "T >= 1 and V >= 1");
  DLLM_HOST_CHECK(K % PBK == 0 && K >= PBK, "K must be a positive multiple of 64");
  DLLM_HOST_CHECK((long)T * K * 2 < (1L << 32) && (long)V * K * 2 < (1L << 32), "operands must be < 4 GiB");
  const int mtiles = (T + 255) / 256, ntv = (V + 255) / 256;
  DLLM_HOST_CHECK(S >= 1 && S <= ntv, "vocabulary ranges: 1 <= S <= ceil(V / 256)");
  const long grid = (long)mtiles * S;
  DLLM_HOST_CHECK(grid < (1L << 31), "grid");
  DLLM_HOST_CHECK(ws != 0 && (long)T * kLmHeadWaves * S * 3 <= ws_floats, "lm_head_logprobs workspace too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lm_head_logprobs_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const bf16*)x, (const bf16*)w,
                     (const int*)targets, (float*)ws, T, V, K, S);
  DLLM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lm_head_logprobs_reduce, dim3((unsigned)mtiles), dim3(256), 0, s, (float*)out, (const float*)ws,
                     (const int*)targets, T, kLmHeadWaves * S);
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
