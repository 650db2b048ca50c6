// qkv_prep: what Qwen2 / Qwen3 add between the qkv projection and RoPE, in place on the dense bf16
// qkv [T, (Hq + 2 Hkv) D] (contract: ops/reference.py qkv_prep).
//   r = f32(qkv[t, s, :]) + f32(bias[s, :])                       (no bias: r = f32(qkv))
//   q slots with q_w, k slots with k_w:  y = bf16(r * rsqrt(mean_D(r^2) + eps) * w)   one rounding
//   every other slot:                    y = bf16(r)
// Head slots that neither the bias nor a norm touches (v without a bias, k without k_w, q without
// q_w) are neither read nor written: the grid runs over the slot range [s0, s1) only.
//
// A pure stream, 2 x bytes of the touched heads: a lane owns one 16-byte vector (8 bf16), a head is
// a group of D / 8 lanes (16 at D = 128, 8 at D = 64), and a token's touched heads are contiguous,
// so a wave moves whole lines.  The sum of squares is reduced inside the lane group with DPP row
// operations (a DPP row is 16 lanes): no LDS, no atomics, no scratch.  The bias and weight vectors
// (a few KB) stay in cache.  One launch for all T rows, nothing allocated, no host synchronisation:
// the kernel is captured into the decode graphs.
#include "common.h"
#include "launchers.h"

namespace dllm {

// DPP controls: quad_perm [1, 0, 3, 2] / [2, 3, 0, 1] (xor 1 / xor 2 inside a quad), row_half_mirror
// (lane i <-> 7 - i of its 8) and row_mirror (i <-> 15 - i of its 16).  After the two quad steps every
// lane of a quad holds the quad's sum, so a mirror step adds the other quad's / the other half's sum:
// every lane of the group ends with the same bits (each step is a two-operand add of the same pair).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false);
  return v + __int_as_float(o);
}

template <int G>   // lanes per head: D / 8
__device__ __forceinline__ float group_sum(float v) {
  static_assert(G == 8 || G == 16, "a head is 8 or 16 lanes");
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  if constexpr (G == 16) v = dpp_add<0x140>(v);
  return v;
}

constexpr int kPrepUnroll = 2;   // 16-byte loads in flight per lane

// nv: touched vectors per token ((s1 - s0) * G), total = T * nv < 2^31.  Vector i of the launch is
// vector c = i % nv of token i / nv; its head slot is s0 + c / G.  total is a multiple of G and every
// stride below is too, so the lanes of a head group are active together.
template <int G>
__global__ void __launch_bounds__(256) qkv_prep_kernel(bf16* __restrict__ qkv, const bf16* __restrict__ bias,
                                                       const bf16* __restrict__ q_w, const bf16* __restrict__ k_w,
                                                       unsigned total, unsigned nv, int row_elems, int s0, int hq,
                                                       int hkv, float eps) {
  constexpr int D = G * 8;
  const unsigned stride = gridDim.x * 256u;
  for (unsigned i0 = blockIdx.x * 256u + threadIdx.x; i0 < total; i0 += kPrepUnroll * stride) {
    bf16x8 x[kPrepUnroll];
    bf16* p[kPrepUnroll];
    unsigned c[kPrepUnroll];
    bool on[kPrepUnroll];
#pragma unroll
    for (int u = 0; u < kPrepUnroll; ++u) {
      const unsigned i = i0 + u * stride;
      on[u] = i < total;                       // no wrap: total < 2^31 and the grid is at most 2^19 threads
      const unsigned t = on[u] ? i / nv : 0u;
      c[u] = on[u] ? i - t * nv : 0u;
      p[u] = qkv + (size_t)t * row_elems + (size_t)s0 * D + (size_t)c[u] * 8;
      if (on[u]) x[u] = *reinterpret_cast<const bf16x8*>(p[u]);
    }
#pragma unroll
    for (int u = 0; u < kPrepUnroll; ++u) {
      const int s = s0 + (int)(c[u] / G);
      const int e = (int)(c[u] % G) * 8;       // first element of this lane inside the head
      const bf16* w = s < hq ? q_w : (s < hq + hkv ? k_w : nullptr);
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = on[u] ? bf2f(x[u][j]) : 0.f;
      if (on[u] && bias) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(bias + (size_t)s * D + e);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += bf2f(b[j]);
      }
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += r[j] * r[j];
      ss = group_sum<G>(ss);                   // every lane of the wave takes part
      if (!on[u]) continue;
      bf16x8 o;
      if (w) {
        const float inv = rsqrtf(ss / (float)D + eps);
        const bf16x8 g = *reinterpret_cast<const bf16x8*>(w + e);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(r[j] * inv * bf2f(g[j]));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(r[j]);
      }
      *reinterpret_cast<bf16x8*>(p[u]) = o;
    }
  }
}

void qkv_prep(uintptr_t qkv, uintptr_t bias, uintptr_t q_w, uintptr_t k_w, int tokens, int hq, int hkv, int d,
              float eps, uintptr_t stream) {
  DLLM_HOST_CHECK(d == 64 || d == 128, "head_dim must be 64 or 128");
  DLLM_HOST_CHECK(tokens >= 0 && hq >= 1 && hkv >= 1, "tokens >= 0, Hq >= 1, Hkv >= 1");
  DLLM_HOST_CHECK(qkv != 0 && ((qkv | bias | q_w | k_w) & 15) == 0, "qkv, bias and norm weights are 16-byte aligned");
  // slots the launch touches: all of them with a bias; else q (with q_w) and / or k (with k_w)
  const int s0 = bias || q_w ? 0 : hq;
  const int s1 = bias ? hq + 2 * hkv : (k_w ? hq + hkv : hq);
  if (tokens == 0 || s1 <= s0) return;
  const int g = d / 8;
  const long nv = (long)(s1 - s0) * g;
  const long total = nv * tokens;
  const long row_elems = (long)(hq + 2 * hkv) * d;
  DLLM_HOST_CHECK(total < (1L << 31) && row_elems < (1L << 31), "tokens x touched vectors must be below 2^31");
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;            // 256 CUs x 8 blocks, grid-stride the rest
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, (bf16*)qkv, (const bf16*)bias,
                       (const bf16*)q_w, (const bf16*)k_w, (unsigned)total, (unsigned)nv, (int)row_elems, s0, hq, hkv,
                       eps);
  };
  if (d == 128) launch(qkv_prep_kernel<16>);
  else launch(qkv_prep_kernel<8>);
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
