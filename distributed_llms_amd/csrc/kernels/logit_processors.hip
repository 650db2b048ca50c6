// Logit processors: repetition / presence / frequency penalties, logit_bias and the min_tokens EOS
// ban, applied in place to the bf16 logits before argmax / sample_rows / token_logprobs read them.
//
// Contract (ops/reference.py apply_logit_processors is the same thing in numpy float32), for every
// token t some rule touches, from the bf16 logit:
//   x = f32(logit[t])
//   if (in_prompt[t] or n_out[t] > 0) and rep != 1:  x = x > 0 ? x / rep : x * rep
//   if n_out[t] > 0:                                  x = x - freq * f32(n_out[t]);  x = x - pres
//   if t has a bias entry:                            x = x + bias[t]
//   if t == eos and the output index being drawn < min_tokens:  x = -inf
//   logit[t] = bf16_rne(x)                            one rounding, whatever subset applied
// Every operation is its own IEEE rounding (no contraction, a correctly rounded divide): the file is
// compiled without fast-math flags and with fp contract off, so the result is bit-equal to numpy's.
// A token no rule touches keeps its bits; a row that did not ask is neither read nor written.
//
// The per-request token statistics live on the device, one STATE ROW of `pitch` int32 words per
// asking request (engine/logit_state.py): word t = output count (bits 0..23) | kBiasBit (t has an
// entry in the row's bias list) | kPromptBit (t occurs in the prompt).  Three kernels keep them
// current and use them:
//   logit_state_update   prefill chunks: reset at position 0, install the bias list, census the chunk
//   apply_logit_processors  the chain above, one 1024-thread workgroup per asking row
//   logit_state_count    after sampling: count the id each asking row drew
//
// procs [rows, kProcWords] int32, one record per row of the step:
//   0 state row (-1: the row did not ask)   1 prompt length   2 flags   3 rep   4 pres   5 freq (f32 bits)
//   6 min_tokens   7 start (position of the chunk's first token; decode rows: unused)
#include "common.h"
#include "launchers.h"

#pragma clang fp contract(off)

namespace dllm {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 1024;
constexpr uint32_t kCountMask = 0x00FFFFFFu;
constexpr uint32_t kBiasBit = 1u << 29;
constexpr uint32_t kPromptBit = 1u << 31;
constexpr int kFlagSample = 1;   // apply the processors to the row and count what it draws
constexpr int kFlagUpdate = 2;   // the row is a prefill chunk: census its tokens

struct RowProcs {
  float rep, pres, freq;
  int eos;        // the banned id (-1: no ban in this step)
};

// The chain for one token.  w: its state word; bias: its entry (read only when has_bias).
__device__ __forceinline__ uint32_t process(uint32_t bits, uint32_t w, const RowProcs& p, int t, bool has_bias,
                                            float bias) {
  const uint32_t cnt = w & kCountMask;
  const bool seen = (w & kPromptBit) != 0u || cnt != 0u;
  const bool rep_on = seen && p.rep != 1.0f;
  const bool ban = t == p.eos;
  if (!(rep_on || cnt != 0u || has_bias || ban)) return bits;
  float x = __uint_as_float(bits << 16);
  if (rep_on) x = x > 0.0f ? x / p.rep : x * p.rep;
  if (cnt != 0u) {
    const float f = p.freq * (float)cnt;
    x = x - f;
    x = x - p.pres;
  }
  if (has_bias) x = x + bias;
  if (ban) x = -INFINITY;
  const bf16 r = f2bf(x);
  return (uint32_t)__builtin_bit_cast(uint16_t, r);
}

__global__ __launch_bounds__(kThreads) void apply_logit_processors_kernel(
    uint16_t* __restrict__ logits, int vocab, long row_stride, const uint32_t* __restrict__ state, int pitch,
    int state_rows, const int32_t* __restrict__ procs, const int32_t* __restrict__ seq_lens, int eos_id,
    const int32_t* __restrict__ bias_n, const int32_t* __restrict__ bias_ids, const float* __restrict__ bias_vals,
    int bias_pitch) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int32_t* pr = procs + (size_t)r * kProcWords;
  const int srow = pr[0];
  if (srow < 0 || srow >= state_rows || !(pr[2] & kFlagSample)) return;
  RowProcs p;
  p.rep = __int_as_float(pr[3]);
  p.pres = __int_as_float(pr[4]);
  p.freq = __int_as_float(pr[5]);
  // the row draws output token number seq_lens[r] - prompt_len (0 = the first)
  p.eos = (eos_id >= 0 && seq_lens[r] - pr[1] < pr[6]) ? eos_id : -1;
  uint16_t* row = logits + (size_t)r * row_stride;
  const uint32_t* st = state + (size_t)srow * pitch;
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int ngroups = (vocab + 7) >> 3, nfull = vocab >> 3;

  // dense pass: every token without a bias entry
  for (int g = tid; g < ngroups; g += kThreads) {
    // the state row is 16-byte aligned and pitch covers the ragged last group
    const u32x4 w0 = *reinterpret_cast<const u32x4*>(st + g * 8);
    const u32x4 w1 = *reinterpret_cast<const u32x4*>(st + g * 8 + 4);
    const bool eos_here = p.eos >= 0 && (p.eos >> 3) == g;
    if (!eos_here && ((w0[0] | w0[1] | w0[2] | w0[3] | w1[0] | w1[1] | w1[2] | w1[3]) & ~kBiasBit) == 0u) continue;
    const bool vec = aligned && g < nfull;
    u32x4 x;
    if (vec) {
      x = *reinterpret_cast<const u32x4*>(row + g * 8);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = g * 8 + 2 * j;
        const uint32_t lo = i < vocab ? row[i] : 0u;
        const uint32_t hi = i + 1 < vocab ? row[i + 1] : 0u;
        x[j] = lo | (hi << 16);
      }
    }
    u32x4 y;
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t w = j < 4 ? w0[j & 3] : w1[j & 3];
      const uint32_t old = (j & 1) ? x[j >> 1] >> 16 : x[j >> 1] & 0xFFFFu;
      const int t = g * 8 + j;
      uint32_t nw = old;
      if (t < vocab && !(w & kBiasBit)) nw = process(old, w, p, t, false, 0.0f);
      changed |= nw != old;
      if (j & 1) y[j >> 1] |= nw << 16;
      else y[j >> 1] = nw;
    }
    if (!changed) continue;
    if (vec) {
      *reinterpret_cast<u32x4*>(row + g * 8) = y;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t old = (j & 1) ? x[j >> 1] >> 16 : x[j >> 1] & 0xFFFFu;
        const uint32_t nw = (j & 1) ? y[j >> 1] >> 16 : y[j >> 1] & 0xFFFFu;
        if (g * 8 + j < vocab && nw != old) row[g * 8 + j] = (uint16_t)nw;
      }
    }
  }
  // a changed group's 16-byte store rewrites its bias tokens' old bits: those stores come first
  __syncthreads();
  // bias pass: one thread per entry of the row's list runs the whole chain for its token
  const int nb = min(bias_n[srow], bias_pitch);
  for (int i = tid; i < nb; i += kThreads) {
    const int t = bias_ids[(size_t)srow * bias_pitch + i];
    if (t < 0 || t >= vocab) continue;
    const uint32_t old = row[t];
    const uint32_t nw = process(old, st[t], p, t, true, bias_vals[(size_t)srow * bias_pitch + i]);
    if (nw != old) row[t] = (uint16_t)nw;
  }
}

__global__ __launch_bounds__(kThreads) void logit_state_update_kernel(
    uint32_t* __restrict__ state, int pitch, int state_rows, int vocab, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ cu_seqlens, const int32_t* __restrict__ procs, int32_t* __restrict__ bias_n,
    int32_t* __restrict__ bias_ids, float* __restrict__ bias_vals, int bias_pitch,
    const int32_t* __restrict__ step_bias_cu, const int32_t* __restrict__ step_bias_ids,
    const float* __restrict__ step_bias_vals) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int32_t* pr = procs + (size_t)r * kProcWords;
  const int srow = pr[0];
  if (srow < 0 || srow >= state_rows || !(pr[2] & kFlagUpdate)) return;
  const int prompt_len = pr[1], start = pr[7];
  uint32_t* st = state + (size_t)srow * pitch;
  if (start == 0) {
    // a request's first chunk (also after a preemption): its own state row starts from nothing
    for (int i = tid * 4; i < pitch; i += kThreads * 4) *reinterpret_cast<u32x4*>(st + i) = u32x4{0u, 0u, 0u, 0u};
    const int b0 = step_bias_cu[r];
    const int nb = min(step_bias_cu[r + 1] - b0, bias_pitch);
    if (tid == 0) bias_n[srow] = nb;
    for (int i = tid; i < nb; i += kThreads) {
      bias_ids[(size_t)srow * bias_pitch + i] = step_bias_ids[b0 + i];
      bias_vals[(size_t)srow * bias_pitch + i] = step_bias_vals[b0 + i];
    }
    // the zeros reach the device's L2, where the atomics below operate, before any of them
    __threadfence();
    __syncthreads();
    for (int i = tid; i < nb; i += kThreads) {
      const int t = step_bias_ids[b0 + i];
      if (t >= 0 && t < vocab) atomicOr(st + t, kBiasBit);
    }
  }
  const int a = cu_seqlens[r], n = cu_seqlens[r + 1] - a;
  for (int i = tid; i < n; i += kThreads) {
    const int t = ids[a + i];
    if (t < 0 || t >= vocab) continue;
    if (start + i < prompt_len) atomicOr(st + t, kPromptBit);
    else atomicAdd(st + t, 1u);
  }
}

__global__ void logit_state_count_kernel(uint32_t* __restrict__ state, int pitch, int state_rows, int vocab,
                                         const int32_t* __restrict__ ids, const int32_t* __restrict__ procs, int rows) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int32_t* pr = procs + (size_t)r * kProcWords;
  const int srow = pr[0], t = ids[r];
  if (srow < 0 || srow >= state_rows || !(pr[2] & kFlagSample) || t < 0 || t >= vocab) return;
  atomicAdd(state + (size_t)srow * pitch + t, 1u);
}

void check_state(const char* op, uintptr_t state, int pitch, int state_rows, int vocab) {
  DLLM_HOST_CHECK(state_rows >= 1, std::string(op) + ": no state rows");
  DLLM_HOST_CHECK(vocab >= 1 && pitch >= vocab && (pitch & 7) == 0,
                  std::string(op) + ": pitch must be a multiple of 8 that covers the vocabulary");
  DLLM_HOST_CHECK((state & 15) == 0, std::string(op) + ": state must be 16-byte aligned");
}

}  // namespace

void apply_logit_processors(uintptr_t logits, int rows, int vocab, long row_stride, uintptr_t state, int pitch,
                            int state_rows, uintptr_t procs, uintptr_t seq_lens, int eos_id, uintptr_t bias_n,
                            uintptr_t bias_ids, uintptr_t bias_vals, int bias_pitch, uintptr_t stream) {
  if (rows == 0) return;
  check_state("apply_logit_processors", state, pitch, state_rows, vocab);
  DLLM_HOST_CHECK(row_stride >= vocab, "apply_logit_processors: rows must not overlap");
  DLLM_HOST_CHECK(bias_pitch >= 0 && eos_id < vocab, "apply_logit_processors: bias pitch / eos id");
  hipLaunchKernelGGL(apply_logit_processors_kernel, dim3(rows), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), (uint16_t*)logits, vocab, row_stride,
                     (const uint32_t*)state, pitch, state_rows, (const int32_t*)procs, (const int32_t*)seq_lens,
                     eos_id, (const int32_t*)bias_n, (const int32_t*)bias_ids, (const float*)bias_vals, bias_pitch);
  DLLM_HIP_CHECK(hipGetLastError());
}

void logit_state_update(uintptr_t state, int pitch, int state_rows, int vocab, uintptr_t ids, uintptr_t cu_seqlens,
                        uintptr_t procs, int rows, uintptr_t bias_n, uintptr_t bias_ids, uintptr_t bias_vals,
                        int bias_pitch, uintptr_t step_bias_cu, uintptr_t step_bias_ids, uintptr_t step_bias_vals,
                        uintptr_t stream) {
  if (rows == 0) return;
  check_state("logit_state_update", state, pitch, state_rows, vocab);
  DLLM_HOST_CHECK(bias_pitch >= 0, "logit_state_update: bias pitch");
  hipLaunchKernelGGL(logit_state_update_kernel, dim3(rows), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     (uint32_t*)state, pitch, state_rows, vocab, (const int32_t*)ids, (const int32_t*)cu_seqlens,
                     (const int32_t*)procs, (int32_t*)bias_n, (int32_t*)bias_ids, (float*)bias_vals, bias_pitch,
                     (const int32_t*)step_bias_cu, (const int32_t*)step_bias_ids, (const float*)step_bias_vals);
  DLLM_HIP_CHECK(hipGetLastError());
}

void logit_state_count(uintptr_t state, int pitch, int state_rows, int vocab, uintptr_t ids, uintptr_t procs, int rows,
                       uintptr_t stream) {
  if (rows == 0) return;
  check_state("logit_state_count", state, pitch, state_rows, vocab);
  hipLaunchKernelGGL(logit_state_count_kernel, dim3((rows + 255) / 256), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (uint32_t*)state, pitch, state_rows, vocab,
                     (const int32_t*)ids, (const int32_t*)procs, rows);
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
