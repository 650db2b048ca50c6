// Seeded on-device sampling: temperature / top-k / top-p / draw, one launch, one read of the row.
//
// Contract (ops/reference.py sample_rows is the same thing in float64):
//   temp_e4 <= 0   the row's argmax (first index on ties, NaN never taken, all -inf -> 0)
//   otherwise      NaN counts as -inf, w_i = exp((l_i - l_max) / T), T = temp_e4 * 1e-4
//     top-k        keep x >= the k-th largest value (ties at the threshold all kept)
//     top-p        over the top-k survivors keep value v iff mass{x > v} <= p * Z_k
//     draw         u = (philox4x32_10((pos, 0, 0, 0), seed)[0] >> 8) * 2^-24; the first kept index,
//                  in token order, whose inclusive cumulative kept mass exceeds u * Z_kept
//
// bf16 logits have at most 65,536 distinct values, so both thresholds are exact two-level (high
// byte, low byte) 256-bin radix selections on an order-preserving 16-bit key: no sort.  Masses are
// 2^40-scaled 64-bit integers, so every sum here (LDS atomics, wave reductions) is associative:
// the result does not depend on arrival order, row index or batch size.
//
// One 1024-thread workgroup per row.  A row (up to 131,072 entries) is read once and its keys stay
// in registers (16 x 4 packed VGPRs per thread) for the later passes.  Thread t owns the 8-element
// groups t, t + 1024, ...: a group is one 16-byte load on a 16-byte aligned row and 8 scalar loads
// otherwise (and for the ragged last group).
#include "common.h"
#include "launchers.h"

namespace dllm {
namespace {

typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 1024;
constexpr int kRegIters = 16;            // groups per thread: vocab <= 16 * 1024 * 8
constexpr int kCopies = 16;              // histogram copies per bin (lane & 15): 4 lanes per word at most
constexpr uint32_t kKeyNegInf = 0x007Fu; // key of -inf (and of NaN); 0 marks an index past the row

// bf16 bits -> 16-bit key, increasing with the value.  NaN -> -inf, -0 -> +0.
__device__ __forceinline__ uint32_t key_of(uint32_t b) {
  if (b == 0x8000u) b = 0;
  uint32_t k = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
  return (b & 0x7FFFu) > 0x7F80u ? kKeyNegInf : k;
}

__device__ __forceinline__ float val_of(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu);
  return __uint_as_float(b << 16);
}

// keys of group g (elements 8g .. 8g + 7) from 2-byte loads, two per dword; 0 for indices >= vocab
__device__ __forceinline__ u32x4 load_group(const uint16_t* __restrict__ row, int g, int vocab) {
  u32x4 x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = g * 8 + 2 * j;
    const uint32_t lo = i < vocab ? key_of(row[i]) : 0u;
    const uint32_t hi = i + 1 < vocab ? key_of(row[i + 1]) : 0u;
    x[j] = lo | (hi << 16);
  }
  return x;
}

__device__ __forceinline__ uint32_t key_at(const u32x4& x, int j) {
  return (j & 1) ? x[j >> 1] >> 16 : x[j >> 1] & 0xFFFFu;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, DLLM_WAVE);
  return v;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o, DLLM_WAVE);
    v = t > v ? t : v;
  }
  return v;
}

__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, DLLM_WAVE);
    if (lane >= o) v += t;
  }
  return v;
}

// a wave-uniform value, moved to scalar registers
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 uni(u64 v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// First position, in scan order, at which base + (inclusive sum of arr) exceeds target.  Run by a
// whole wave on an LDS array of 64 * C entries; lane l owns scan positions l*C .. l*C + C - 1.
// DESC: position r is entry 255 - r (a 256-bin histogram walked from the top).  Returns false
// when the sum never exceeds target; else entry index and the sum (base included) of everything
// before it.
template <typename T, int C, bool DESC>
__device__ __forceinline__ bool scan_cross(const T* arr, u64 base, u64 target, int lane, int& entry,
                                           u64& before) {
  u64 v[C];
  u64 s = 0;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int e = DESC ? 255 - (lane * C + j) : lane * C + j;
    v[j] = (u64)arr[e];
    s += v[j];
  }
  const u64 incl = base + wave_incl_scan_u64(s, lane);
  const u64 hit = __ballot(incl > target);
  if (hit == 0) return false;
  const int src = __ffsll((long long)hit) - 1;
  u64 a = incl - s;
  int found = -1;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    if (found < 0) {
      if (a + v[j] > target) found = DESC ? 255 - (lane * C + j) : lane * C + j;
      else a += v[j];
    }
  }
  entry = uni(__shfl(found, src, DLLM_WAVE));
  before = uni(__shfl(a, src, DLLM_WAVE));
  return true;
}

// sum of a 256-entry LDS array (whole wave)
template <typename T>
__device__ __forceinline__ u64 sum_all(const T* arr, int lane) {
  u64 s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += (u64)arr[lane * 4 + j];
  return uni(wave_sum_u64(s));
}

__device__ __forceinline__ uint32_t philox4x32_10_first(uint32_t c0, uint32_t k0, uint32_t k1) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// f(it) for the row's iterations: fully unrolled over the capacity, so x[it] is a register, never
// an indexed array
template <typename F>
__device__ __forceinline__ void for_iters(int nit, F&& f) {
#pragma unroll
  for (int it = 0; it < kRegIters; ++it)
    if (it < nit) f(it);
}

// Pass 1 of both kernels, the only read of the row: its keys into x, and the thread's best
// key << 32 | ~index (the larger key, then the smaller index, wins a plain max; 0: no entry).
__device__ __forceinline__ u64 load_row_keys(u32x4 (&x)[kRegIters], const uint16_t* __restrict__ row, int vocab,
                                             bool aligned, int tid, int ngroups, int nit) {
  u64 best = 0;
  if (aligned) {
    // every full group's 16-byte load is issued before the first conversion waits on one
    const int nfull = vocab >> 3;
#pragma unroll
    for (int it = 0; it < kRegIters; ++it) {
      const int g = it * kThreads + tid;
      x[it] = u32x4{0u, 0u, 0u, 0u};
      if (g < nfull) x[it] = *reinterpret_cast<const u32x4*>(row + g * 8);
    }
#pragma unroll
    for (int it = 0; it < kRegIters; ++it) {
      const int g = it * kThreads + tid;
      if (g < nfull) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[it][j] = key_of(x[it][j] & 0xFFFFu) | (key_of(x[it][j] >> 16) << 16);
      } else if (g < ngroups) {
        x[it] = load_group(row, g, vocab);   // the ragged last group
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < kRegIters; ++it) {
      const int g = it * kThreads + tid;
      x[it] = u32x4{0u, 0u, 0u, 0u};
      if (g < ngroups) x[it] = load_group(row, g, vocab);
    }
  }
  for_iters(nit, [&](int it) {
    const int g = it * kThreads + tid;
    if (g < ngroups) {
      const u32x4 xg = x[it];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t k = key_at(xg, j);
        const u64 cand = ((u64)k << 32) | (uint32_t)~(uint32_t)(g * 8 + j);
        if (k != 0 && cand > best) best = cand;
      }
    }
  });
  return best;
}

// An empty asm per word makes x opaque to the compiler at this point: what a pass derives from x
// (keys, masses, index words) is then not common to the passes before and after it
__device__ __forceinline__ void launder_keys(u32x4 (&x)[kRegIters]) {
#pragma unroll
  for (int it = 0; it < kRegIters; ++it) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t t = x[it][j];
      asm volatile("" : "+v"(t));
      x[it][j] = t;
    }
  }
}

// floor(2^40 * exp2((val(k) - lmax) * (c + c_lo))) of key k; exactly 2^40 for the row's maximum
__device__ __forceinline__ u64 mass_q40(uint32_t k, uint32_t maxkey, float lmax, float c, float c_lo) {
  if (k == maxkey) return 1ull << 40;
  // floor(w * 2^40) from two 20-bit halves (both products and the remainder are exact in f32)
  const float d = val_of(k) - lmax;
  const float arg = d == -INFINITY ? d : fmaf(d, c, d * c_lo);   // -inf * c_lo may be +inf
  const float w20 = __builtin_amdgcn_exp2f(arg) * 0x1p20f;
  const uint32_t hi = (uint32_t)w20;
  const uint32_t lo = (uint32_t)((w20 - (float)hi) * 0x1p20f);
  return ((u64)hi << 20) | lo;
}

struct SampleShared {
  uint32_t cnt_h[256 * kCopies];   // histogram copies: [bin][lane & 15]
  u64 mass_h[256 * kCopies];       // the final pass reuses the first 256 entries as per-wave sums
  uint32_t cnt1[256], cnt2[256];   // level 1 (high byte) and level 2 (low byte of one bin)
  u64 mass1[256], mass2[256];
  u64 red[16];
};

__device__ __forceinline__ void sample_row(SampleShared& sh, int32_t* __restrict__ out,
                                           const uint16_t* __restrict__ row, int vocab, bool aligned, int temp_e4,
                                           int top_k, int top_p_e4, u64 seed, int pos, const float* uniform) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ngroups = (vocab + 7) >> 3;
  const int nit = (ngroups + kThreads - 1) / kThreads;

  u32x4 x[kRegIters];
  // The passes below recompute keys and masses from x on purpose.  Without this the compiler
  // treats them as common to all passes (and invariant in the threshold loop) and tries to keep
  // all 128 of a thread's masses live: hundreds of spills.  An empty asm makes x opaque per pass.
  auto launder = [&]() { launder_keys(x); };

  // ---- pass 1: the only read of the row; max key and its first index
  u64 best = load_row_keys(x, row, vocab, aligned, tid, ngroups, nit);
  best = wave_max_u64(best);
  if (lane == 0) sh.red[wid] = best;
  __syncthreads();
  best = sh.red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) best = sh.red[w] > best ? sh.red[w] : best;
  best = uni(best);
  const uint32_t maxkey = (uint32_t)(best >> 32);
  const int argidx = (int)~(uint32_t)best;
  // greedy rows and rows without a finite-or-+inf entry end here (workgroup-uniform branch)
  if (temp_e4 <= 0 || maxkey == kKeyNegInf) {
    if (tid == 0) *out = argidx;
    return;
  }

  const float lmax = val_of(maxkey);
  // log2(e) / T as a float pair: the exponent's argument then carries one rounding, not two
  const double cd = 1.4426950408889634 * 1e4 / (double)temp_e4;
  const float c = (float)cd, c_lo = (float)(cd - (double)c);
  auto massq = [&](uint32_t k) -> u64 { return mass_q40(k, maxkey, lmax, c, c_lo); };

  // One 256-bin histogram over the keys >= minkey: of their high byte (sel < 0), or of the low
  // byte of those whose high byte is sel.  Counts (top-k) or masses (top-p): the count passes need
  // no exp2.  Ends with the copies summed into (cnt, mass).
  auto hist_pass = [&](int sel, bool with_mass, uint32_t minkey, uint32_t* cnt, u64* mass) {
    for (int i = tid; i < 256 * kCopies; i += kThreads) {
      sh.cnt_h[i] = 0;
      sh.mass_h[i] = 0;
    }
    __syncthreads();
    launder();
    for_iters(nit, [&](int it) {
      const int g = it * kThreads + tid;
      if (g < ngroups) {
        const u32x4 xg = x[it];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t k = key_at(xg, j);
          const int hb = (int)(k >> 8);
          if (k >= minkey && (sel < 0 || hb == sel)) {
            const int slot = (sel < 0 ? hb : (int)(k & 255u)) * kCopies + (tid & (kCopies - 1));
            if (with_mass) {
              const u64 q = massq(k);
              if (q) atomicAdd(&sh.mass_h[slot], q);
            } else {
              atomicAdd(&sh.cnt_h[slot], 1u);
            }
          }
        }
      }
    });
    __syncthreads();
    if (tid < 256) {
      uint32_t cs = 0;
      u64 ms = 0;
#pragma unroll
      for (int i = 0; i < kCopies; ++i) {
        cs += sh.cnt_h[tid * kCopies + i];
        ms += sh.mass_h[tid * kCopies + i];
      }
      cnt[tid] = cs;
      mass[tid] = ms;
    }
    __syncthreads();
  };

  // ---- thresholds.  Every wave walks the same LDS histograms and reaches the same decisions, so
  // the branches below are workgroup-uniform and nothing has to be published.  One histogram loop
  // serves the (at most four) passes: top-k on counts at level 1 and inside its bin, then top-p on
  // the masses of the top-k survivors (keys >= tau) at level 1 and inside its bin.
  const bool kact = top_k > 0 && top_k < vocab;
  const bool pact = top_p_e4 < 10000;
  uint32_t tau = 1;            // smallest kept key (0 marks an index past the row)
  if (kact || pact) {
    const u64 kth = (u64)top_k - 1;   // the k-th largest: the first inclusive count above k - 1
    const u64 p = top_p_e4 > 0 ? (u64)top_p_e4 : 0ull;
    int stage = kact ? 0 : 2, sel = -1, bin = 0, low = 0;
    u64 above = 0, tgt = 0, unused = 0;
#pragma unroll 1
    for (;;) {
      hist_pass(sel, stage >= 2, tau, sel < 0 ? sh.cnt1 : sh.cnt2, sel < 0 ? sh.mass1 : sh.mass2);
      if (stage == 0) {
        scan_cross<uint32_t, 4, true>(sh.cnt1, 0, kth, lane, bin, above);
        sel = bin;
        stage = 1;
      } else if (stage == 1) {
        scan_cross<uint32_t, 4, true>(sh.cnt2, above, kth, lane, low, unused);
        tau = ((uint32_t)bin << 8) | (uint32_t)low;
        if (!pact) break;
        sel = -1;
        stage = 2;
      } else if (stage == 2) {
        const u64 zk = sum_all(sh.mass1, lane);
        tgt = (zk / 10000ull) * p + ((zk % 10000ull) * p) / 10000ull;   // floor(p * Z_k)
        if (!scan_cross<u64, 4, true>(sh.mass1, 0, tgt, lane, bin, above)) break;   // all survivors kept
        sel = bin;
        stage = 3;
      } else {
        scan_cross<u64, 4, true>(sh.mass2, above, tgt, lane, low, unused);
        tau = ((uint32_t)bin << 8) | (uint32_t)low;
        break;
      }
    }
  }

  // ---- draw
  uint32_t m24;
  if (uniform) {
    const float uf = fminf(fmaxf(*uniform, 0.f), 1.f) * 16777216.f;
    m24 = uf >= 16777215.f ? 16777215u : (uint32_t)uf;
  } else {
    m24 = philox4x32_10_first((uint32_t)pos, (uint32_t)seed, (uint32_t)(seed >> 32)) >> 8;
  }

  // kept mass of one group, in index order
  auto group_mass = [&](const u32x4& xg) -> u64 {
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = key_at(xg, j);
      if (k >= tau) s += massq(k);
    }
    return s;
  };

  // per (iteration, wave) kept mass: entry it * 16 + wid covers 512 consecutive indices, and the
  // entries are in index order
  u64* wsum = sh.mass_h;
  if (tid < kRegIters * 16) wsum[tid] = 0;
  __syncthreads();
  u64 ztot = 0;
  launder();
  for_iters(nit, [&](int it) {
    const int g = it * kThreads + tid;
    u64 s = 0;
    if (g < ngroups) s = group_mass(x[it]);
    if (__ballot(s != 0) != 0) {
      s = wave_sum_u64(s);
      if (lane == 0) wsum[it * 16 + wid] = s;
      ztot += s;
    }
  });
  // Z_kept: the sum of the per-wave sums
  if (lane == 0) sh.red[wid] = ztot;
  __syncthreads();
  u64 zkept = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) zkept += sh.red[w];
  zkept = uni(zkept);

  // cum > u * Z  <=>  cum > floor(Z * m24 / 2^24) for integer cum
  const u64 target = (zkept >> 24) * m24 + (((zkept & 0xFFFFFFull) * m24) >> 24);
  int entry = 0;
  u64 before = 0;
  const bool found = scan_cross<u64, kRegIters * 16 / 64, false>(wsum, 0, target, lane, entry, before);
  if (!found) {   // cannot happen with integer masses (target < Z); the max is always kept
    if (tid == 0) *out = argidx;
    return;
  }
  if (wid != (entry & 15)) return;
  const int it_hit = entry >> 4;
  launder();
  for_iters(nit, [&](int it) {
    if (it != it_hit) return;
    const int g = it * kThreads + tid;
    u32x4 xg = u32x4{0u, 0u, 0u, 0u};
    if (g < ngroups) xg = x[it];
    const u64 s = group_mass(xg);
    const u64 incl = before + wave_incl_scan_u64(s, lane);
    const u64 hit = __ballot(incl > target);
    if (hit == 0) {   // unreachable: scan_cross found the crossing inside this wave's entry
      if (lane == 0) *out = argidx;
      return;
    }
    if (lane == __ffsll((long long)hit) - 1) {
      u64 a = incl - s;
      int id = argidx;
      bool done = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t k = key_at(xg, j);
        if (!done && k >= tau) {
          a += massq(k);
          if (a > target) {
            id = g * 8 + j;
            done = true;
          }
        }
      }
      *out = id;
    }
  });
}

__global__ void __launch_bounds__(1024) sample_rows_kernel(int32_t* __restrict__ out, const bf16* __restrict__ logits,
                                                           int vocab, long row_stride,
                                                           const int32_t* __restrict__ params,
                                                           const u64* __restrict__ seeds,
                                                           const int32_t* __restrict__ pos,
                                                           const float* __restrict__ uniforms) {
  __shared__ SampleShared sh;
  const int b = blockIdx.x;
  const uint16_t* row = reinterpret_cast<const uint16_t*>(logits) + (size_t)b * row_stride;
  const bool aligned = (((uintptr_t)row) & 15) == 0;
  const int temp_e4 = params[b * 3], top_k = params[b * 3 + 1], top_p_e4 = params[b * 3 + 2];
  sample_row(sh, out + b, row, vocab, aligned, temp_e4, top_k, top_p_e4, seeds[b], pos[b],
             uniforms ? uniforms + b : nullptr);
}

// ---------------------------------------------------------------------------------------------
// Per-token log-probabilities of the model's distribution (no temperature, top-k or top-p):
// ops/reference.py token_logprobs is the same thing in float64.
//   m = row maximum (NaN counts as -inf), Z = sum_j exp(x_j - m) with exactly 1 for x_j == m,
//   lp_i = (x_i - m) - ln Z with x_i - m = 0 where x_i == m; every lp is -inf when m is -inf
//   want < 0   the row is skipped: chosen = 0, top_ids = -1, top_lp = 0
//   want = n   chosen = lp[ids[b]] (-inf for an id outside the row); the first min(n, n_max, vocab)
//              top slots hold the largest entries by decreasing value, then increasing index; the
//              rest hold -1 / 0
// Z is the integer sum of the sampler's 2^40-scaled masses at T = 1, so a row's outputs do not
// depend on its batch, its row index or the launch.  The top entries come from n rounds of a
// workgroup max over key << 32 | ~index: unique per entry, so the order needs no tie rule.  A
// thread keeps its best composite below the last winner, so only the winner's owner has to look at
// its 128 entries again: it hands them to its wave through LDS, two entries per lane (one lane
// walking all 128 measured 4.5 us per round; profiles/logprobs.md).
struct LogprobShared {
  u64 red[2][16];   // alternating buffers: one barrier per round
  u64 zred[16];
  float lnz;
  uint32_t scan[16][kRegIters * 4];   // per wave: the owner's packed keys
};

__global__ void __launch_bounds__(1024) token_logprobs_kernel(float* __restrict__ chosen, int32_t* __restrict__ top_ids,
                                                              float* __restrict__ top_lp,
                                                              const bf16* __restrict__ logits, int vocab,
                                                              long row_stride, const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ want, int n_max) {
  __shared__ LogprobShared sh;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int n = want[b];
  n = n > n_max ? n_max : n;
  n = n > vocab ? vocab : n;
  int32_t* tids = top_ids + (size_t)b * n_max;
  float* tlps = top_lp + (size_t)b * n_max;
  if (tid < n_max && tid >= n) {   // n < 0: every slot
    tids[tid] = -1;
    tlps[tid] = 0.f;
  }
  if (n < 0) {   // workgroup-uniform
    if (tid == 0) chosen[b] = 0.f;
    return;
  }

  const uint16_t* row = reinterpret_cast<const uint16_t*>(logits) + (size_t)b * row_stride;
  const bool aligned = (((uintptr_t)row) & 15) == 0;
  const int ngroups = (vocab + 7) >> 3;
  const int nit = (ngroups + kThreads - 1) / kThreads;

  u32x4 x[kRegIters];
  // as in sample_row: x opaque per pass, so no pass's per-entry values are kept live for another
  auto launder = [&]() { launder_keys(x); };
  // the workgroup's largest composite; round r uses buffer r & 1
  auto block_max = [&](u64 v, int buf) -> u64 {
    v = wave_max_u64(v);
    if (lane == 0) sh.red[buf][wid] = v;
    __syncthreads();
    u64 m = sh.red[buf][0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = sh.red[buf][w] > m ? sh.red[buf][w] : m;
    return uni(m);
  };

  // ---- pass 1: the only read of the row; the thread's best entry, then the row's
  u64 mine = load_row_keys(x, row, vocab, aligned, tid, ngroups, nit);
  u64 win = block_max(mine, 0);
  const uint32_t maxkey = (uint32_t)(win >> 32);
  const bool dead = maxkey == kKeyNegInf;   // no entry above -inf: every lp is -inf
  const float lmax = val_of(maxkey);

  // ---- Z and ln Z
  if (!dead) {
    const double cd = 1.4426950408889634;   // log2(e): T = 1
    const float c = (float)cd, c_lo = (float)(cd - (double)c);
    u64 z = 0;
    launder();
    for_iters(nit, [&](int it) {
      const int g = it * kThreads + tid;
      if (g < ngroups) {
        const u32x4 xg = x[it];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t k = key_at(xg, j);
          if (k != 0) z += mass_q40(k, maxkey, lmax, c, c_lo);
        }
      }
    });
    z = wave_sum_u64(z);
    if (lane == 0) sh.zred[wid] = z;
    __syncthreads();
    if (tid == 0) {
      u64 zt = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) zt += sh.zred[w];
      sh.lnz = (float)log((double)zt * 0x1p-40);   // Z >= 1: the maximum's own mass
    }
    __syncthreads();
  }
  const float lnz = dead ? 0.f : sh.lnz;
  auto lp_of = [&](uint32_t k) -> float {
    if (dead) return -INFINITY;
    const float d = k == maxkey ? 0.f : val_of(k) - lmax;   // -inf below a +inf maximum
    return d - lnz;
  };

  // ---- the chosen token: its owner holds the key in registers
  const int id = ids[b];
  if (id < 0 || id >= vocab) {
    if (tid == 0) chosen[b] = -INFINITY;
  } else if (tid == ((id >> 3) & (kThreads - 1))) {
    const int it_c = (id >> 3) / kThreads, j_c = id & 7;
    uint32_t kc = 0;
    for_iters(nit, [&](int it) {
      if (it != it_c) return;
      const u32x4 xg = x[it];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j == j_c) kc = key_at(xg, j);
    });
    chosen[b] = lp_of(kc);
  }

  // ---- the n largest entries
#pragma unroll 1
  for (int r = 0; r < n; ++r) {
    if (tid == 0) {
      tids[r] = (int)~(uint32_t)win;
      tlps[r] = lp_of((uint32_t)(win >> 32));
    }
    if (r + 1 == n) break;
    const u64 own = __ballot(mine == win);   // one lane of one wave
    if (own != 0) {                           // wave-uniform: the owner's wave finds its next best entry
      const int src = __ffsll((long long)own) - 1;
      uint32_t* sc = sh.scan[wid];
      if (lane == src) {
#pragma unroll
        for (int it = 0; it < kRegIters; ++it) {
#pragma unroll
          for (int j = 0; j < 4; ++j) sc[it * 4 + j] = x[it][j];   // zeros past the row
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      // lane l: dword l, the entries 2 * (l & 3) and + 1 of the owner's group in iteration l >> 2
      const uint32_t d = sc[lane];
      const int g = (lane >> 2) * kThreads + (wid * 64 + src);
      u64 nb = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t k = h ? d >> 16 : d & 0xFFFFu;
        const u64 cand = ((u64)k << 32) | (uint32_t)~(uint32_t)(g * 8 + 2 * (lane & 3) + h);
        if (k != 0 && cand < win && cand > nb) nb = cand;
      }
      nb = wave_max_u64(nb);
      if (lane == src) mine = nb;
    }
    win = block_max(mine, (r + 1) & 1);
  }
}

}  // namespace

void sample_rows(uintptr_t out_ids, uintptr_t logits, int rows, int vocab, long row_stride, uintptr_t params,
                 uintptr_t seeds, uintptr_t pos, uintptr_t uniforms, uintptr_t stream) {
  if (rows == 0) return;
  DLLM_HOST_CHECK(vocab >= 1 && vocab <= kRegIters * kThreads * 8, "sample_rows: vocab must be in [1, 131072]");
  DLLM_HOST_CHECK(row_stride >= 0, "sample_rows: row stride must not be negative");
  DLLM_HOST_CHECK((seeds & 7) == 0, "sample_rows: seeds must be 8-byte aligned");
  hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     (int32_t*)out_ids, (const bf16*)logits, vocab, row_stride, (const int32_t*)params,
                     (const u64*)seeds, (const int32_t*)pos, (const float*)uniforms);
  DLLM_HIP_CHECK(hipGetLastError());
}

void token_logprobs(uintptr_t chosen, uintptr_t top_ids, uintptr_t top_lp, uintptr_t logits, int rows, int vocab,
                    long row_stride, uintptr_t ids, uintptr_t want, int n_max, uintptr_t stream) {
  if (rows == 0) return;
  DLLM_HOST_CHECK(vocab >= 1 && vocab <= kRegIters * kThreads * 8, "token_logprobs: vocab must be in [1, 131072]");
  DLLM_HOST_CHECK(row_stride >= 0, "token_logprobs: row stride must not be negative");
  DLLM_HOST_CHECK(n_max >= 0 && n_max <= kMaxLogprobs, "token_logprobs: n_max must be in [0, 20]");
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(rows), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     (float*)chosen, (int32_t*)top_ids, (float*)top_lp, (const bf16*)logits, vocab, row_stride,
                     (const int32_t*)ids, (const int32_t*)want, n_max);
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
