// Weight-only int4 (W4A16) decode GEMM: y[M, N] = x[M, K] . wd[N, K]^T with bf16 x, f32 accumulate and
// wd[n, k] = (u[n, k] - 8) * s[n, k / 128]: 4-bit codes u in 0..15, one bf16 scale per 128 consecutive k of
// a row (contract: ops/reference.py linear_w4).  At decode-sized M every projection is a weight stream;
// half a byte per weight quarters it.
//
// Weight layout (packed once at load, ops/int4.py pack): MFMA-fragment-major.  For each 16-row weight tile
// t and each 128-k group g one contiguous 1 KiB block (t * K / 128 + g); lane l of a wave owns 16 bytes of
// it -- row l % 16, and in 32-bit word j (the K-step of v_mfma_f32_16x16x32_bf16) the eight k at
// 32 j + 8 (l / 16) + e, code e at bit 4 (e / 2) + 16 (e % 2).  So one 16-byte load hands a lane one whole
// scale group of one row, and (w >> 4 p) & 0x000F000F is the fragment's element pair (2 p, 2 p + 1), each in
// its 16-bit half.  Scales are bf16 [N / 16, K / 128, 16]: the four a lane needs are 8 adjacent bytes.
//
// gemm_w4a16 (grid: N / 128 column tiles x ceil(M / 64) row tiles x K slices; 256 threads):
//  * weights go global -> registers with one nontemporal 16-byte load per (16-row tile, group), never
//    through LDS; each wave owns 32 of the tile's 128 weight rows;
//  * code -> bf16 with no integer-to-float conversion: code | 0x4300 is the bf16 value 128 + code, exactly;
//    the offset 136 comes off as f32 (the bf16 bits shifted into a float), where the difference -8..7 is
//    exact, and the pair is packed back to bf16;
//  * the weight fragment is the MFMA A operand, so the accumulators hold y^T: a lane has 4 consecutive n of
//    one m and stores them as 8 bytes (16 bytes of f32 into a split-K slab);
//  * the scale is applied once per (group, accumulator register): four MFMAs into a group accumulator,
//    then acc += s * group_acc -- never per element;
//  * x tiles (64 rows x 128 k bf16, 16 KiB) go through a two-buffer LDS ring by LDS-DMA
//    (global_load_lds_dwordx4, lane-linear 1 KiB = 4 rows per wave instruction) with the bank swizzle
//    chunk ^ (row & 15) on the source address and on the ds_read_b128 address; group g + 1's tile and
//    weights are in flight while group g is multiplied, one barrier per group;
//  * CT (1, 2 or 4) 16-row x fragments per tile: M <= 16 / <= 32 stage and multiply only those rows.  Rows
//    past M read row M - 1 (in bounds) into accumulator columns that are never stored;
//  * split-K: slices write f32 partials [S, M, N] to the workspace, w4_reduce sums them in slice order and
//    rounds once -- no atomics, the same bits on every launch, graph-capturable.  One slice stores bf16.
//
// Zero-point variant (template parameter ZP; AWQ / GPTQ checkpoints, ops/int4.py from_checkpoint):
// wd[n, k] = (u[n, k] - z[n, k / 128]) * f32(s[n, k / 128]) with an integer z in 0..15 and an f16 or bf16 s.  Both
// live in ONE dword per (row, group), u32 [N / 16, K / 128, 16] in place of the bf16 scales: the f32 value of s
// (exact for f16 and bf16, whose low 13 mantissa bits are then zero) with z in bits 0..3 -- so the kernels never
// see the scale's dtype, s is `dword & ~15` and z is `dword & 15`.  A lane needs the scales of its four
// accumulator rows 4 (l / 16) .. + 3 (one 16-byte load, as the symmetric kernel's 8-byte one) and the zero of its
// fragment row l % 16 (one more dword of the same 64-byte line).  code | 0x4300 stays; the offset that comes off in
// f32 is 128 + z, the difference -15..15 is exact in bf16, and the scale is still applied once per group and
// accumulator register.  The symmetric instantiations (ZP = false) are the code they were.
//
// dequant_w4: the whole weight to bf16_rne(wd) in plain [N, K] order for the large-M route (the existing bf16
// GEMMs then serve it): one wave per 1 KiB block, every store instruction writes 4 rows x 256 bytes.
#include "common.h"
#include "launch_host.h"
#include "launchers.h"

namespace dllm {

namespace {
typedef uint32_t u32x4q __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_vptr_q;
typedef __attribute__((address_space(1))) void* glb_vptr_q;

constexpr int QBM = 64, QBN = 128, QG = 128;       // x rows / weight rows per tile, k per scale group
constexpr int QXTILE = QBM * QG;                    // bf16 elements of one x tile (16 KiB)

// one K-step's A fragment (8 bf16 of one weight row) from its packed word
// (`off`: 128 + the zero point)
__device__ __forceinline__ bf16x8 w4_frag(uint32_t w, float off) {
  bf16x8 f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t pair = ((w >> (4 * p)) & 0x000F000Fu) | 0x43004300u;      // bf16 (128 + u) x 2
    const float lo = __uint_as_float(pair << 16) - off, hi = __uint_as_float(pair & 0xFFFF0000u) - off;
    f[2 * p] = f2bf(lo);
    f[2 * p + 1] = f2bf(hi);
  }
  return f;
}
}  // namespace

// ZP: `Scv` is the u32 scale | zero array, else the bf16 scales
template <int CT, bool SPLIT, bool ZP>
__global__ void __launch_bounds__(256) gemm_w4a16_kernel(bf16* __restrict__ C, float* __restrict__ P,
                                                         const bf16* __restrict__ X, const uint8_t* __restrict__ Wp,
                                                         const void* __restrict__ Scv, int M, int N, int K, int gps) {
  const bf16* __restrict__ Sc = static_cast<const bf16*>(Scv);
  const uint32_t* __restrict__ Sz = static_cast<const uint32_t*>(Scv);
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * QXTILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * QBN, m0 = blockIdx.y * QBM, split = blockIdx.z;
  const int G = K / QG;
  const int g0 = split * gps, g1 = min(G, g0 + gps);
  const size_t t0 = (size_t)(n0 + 32 * wv) / 16;     // this wave's first 16-row weight tile

  // x tile of group g -> LDS buffer `buf`: wave instruction ii = wv + 4 it covers tile rows 4 ii .. 4 ii + 3
  const bf16* xsrc[CT];
#pragma unroll
  for (int it = 0; it < CT; ++it) {
    const int row = 4 * (wv + 4 * it) + fq;
    xsrc[it] = X + (size_t)min(m0 + row, M - 1) * K + ((fr ^ (row & 15)) * 8);
  }
  auto stage = [&](int buf, int g) {
#pragma unroll
    for (int it = 0; it < CT; ++it)
      __builtin_amdgcn_global_load_lds((glb_vptr_q)(xsrc[it] + g * QG),
                                       (lds_vptr_q)(smem + buf * QXTILE + (wv + 4 * it) * 512), 16, 0, 0);
  };
  u32x4q wq[2];
  bf16x4 sq[2];
  u32x4q zq[2];           // ZP: the four scale | zero dwords of the accumulator rows, and the fragment row's
  uint32_t zr[2];
  auto load_w = [&](int g) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const size_t blk = (t0 + a) * G + g;
      wq[a] = __builtin_nontemporal_load(reinterpret_cast<const u32x4q*>(Wp + blk * 1024) + lane);
      if constexpr (ZP) {
        zq[a] = *reinterpret_cast<const u32x4q*>(Sz + blk * 16 + 4 * fq);
        zr[a] = Sz[blk * 16 + fr];
      } else {
        sq[a] = *reinterpret_cast<const bf16x4*>(Sc + blk * 16 + 4 * fq);
      }
    }
  };

  f32x4 acc[2][CT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[a][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, g0);
  load_w(g0);
  for (int g = g0; g < g1; ++g) {
    const int cur = (g - g0) & 1;
    // this wave's loads of group g (x pieces and weights) have landed; after the barrier so have everyone's,
    // and every wave is done reading the other buffer (group g - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const u32x4q wc[2] = {wq[0], wq[1]};
    const bf16x4 sc[2] = {sq[0], sq[1]};
    const u32x4q zc[2] = {zq[0], zq[1]};
    float off[2] = {136.f, 136.f};
    if constexpr (ZP) {
      off[0] = (float)(128u + (zr[0] & 15u));
      off[1] = (float)(128u + (zr[1] & 15u));
    }
    if (g + 1 < g1) {
      stage(cur ^ 1, g + 1);
      load_w(g + 1);
    }
    const bf16* xs = smem + cur * QXTILE;
    f32x4 ga[2][CT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) ga[a][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8 fb[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        fb[ct] = *reinterpret_cast<const bf16x8*>(xs + (ct * 16 + fr) * QG + (((4 * j + fq) ^ fr) * 8));
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const bf16x8 fa = w4_frag(wc[a][j], off[a]);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          ga[a][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[ct], ga[a][ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s = ZP ? __uint_as_float(zc[a][i] & ~15u) : bf2f(sc[a][i]);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[a][ct][i] += s * ga[a][ct][i];
      }
  }

  // y^T fragments: lane holds n = tile row 4 fq + 0..3 of column m = ct * 16 + fr
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int m = m0 + ct * 16 + fr, n = n0 + 32 * wv + 16 * a + 4 * fq;
      if (m >= M) continue;
      if constexpr (SPLIT) {
        *reinterpret_cast<f32x4*>(P + ((size_t)split * M + m) * N + n) = acc[a][ct];
      } else {
        const bf16x4 o = {f2bf(acc[a][ct][0]), f2bf(acc[a][ct][1]), f2bf(acc[a][ct][2]), f2bf(acc[a][ct][3])};
        *reinterpret_cast<bf16x4*>(C + (size_t)m * N + n) = o;
      }
    }
}

// y = bf16(sum over the S slabs [M, N] of f32 partials, in slice order); mn4 = M N / 4
__global__ void __launch_bounds__(256) w4_reduce_kernel(bf16* __restrict__ C, const float* __restrict__ P, int S,
                                                        size_t mn4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mn4) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(P);
  f32x4 v = p[i];
  for (int s = 1; s < S; ++s) v += p[s * mn4 + i];
  const bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
  reinterpret_cast<bf16x4*>(C)[i] = o;
}

// one wave per (16-row tile, group) block; store `it` writes rows 4 it .. 4 it + 3, 16 chunks of 8 k each
template <bool ZP>
__global__ void __launch_bounds__(256) dequant_w4_kernel(bf16* __restrict__ W, const uint32_t* __restrict__ Wp,
                                                         const void* __restrict__ Scv, int K, size_t nblk) {
  const int lane = threadIdx.x & 63;
  const size_t blk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nblk) return;
  const int G = K / QG;
  const size_t t = blk / G, g = blk % G;
  const int c = lane & 15, j = c >> 2, q = c & 3;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = 4 * it + (lane >> 4);
    const uint32_t w = Wp[blk * 256 + (r + 16 * q) * 4 + j];
    float s;
    int z = 8;
    if constexpr (ZP) {
      const uint32_t d = static_cast<const uint32_t*>(Scv)[blk * 16 + r];
      s = __uint_as_float(d & ~15u);
      z = (int)(d & 15u);
    } else {
      s = bf2f(static_cast<const bf16*>(Scv)[blk * 16 + r]);
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf((float)((int)((w >> (4 * (e >> 1) + 16 * (e & 1))) & 15u) - z) * s);
    *reinterpret_cast<bf16x8*>(W + (t * 16 + r) * K + g * QG + c * 8) = o;
  }
}

int gemm_w4a16(uintptr_t c, uintptr_t x, uintptr_t wp, uintptr_t scale, uintptr_t ws, long ws_floats, int M, int N,
               int K, int splits, int zp, uintptr_t stream) {
  DLLM_HOST_CHECK(M >= 1 && M <= (1 << 20), "1 <= M <= 2^20");
  DLLM_HOST_CHECK(N >= QBN && N % QBN == 0 && K >= QG && K % QG == 0, "N % 128 and K % 128");
  DLLM_HOST_CHECK(c != 0 && x != 0 && wp != 0 && scale != 0, "null operand");
  const SplitK p = splitk_plan(K, QG, splits, 0);
  DLLM_HOST_CHECK(p.S <= 65535, "K slices");
  splitk_check_ws(p, ws, ws_floats, M, N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(N / QBN, (M + QBM - 1) / QBM, p.S);
  dispatch_value<1, 2, 4>(M <= 16 ? 1 : M <= 32 ? 2 : 4, "gemm_w4a16: column fragments", [&](auto ct) {
    dispatch_value<0, 1>(p.S > 1, "gemm_w4a16: split", [&](auto sp) {
      dispatch_value<0, 1>(zp != 0, "gemm_w4a16: zero points", [&](auto z) {
        hipLaunchKernelGGL(
            (gemm_w4a16_kernel<decltype(ct)::value, decltype(sp)::value != 0, decltype(z)::value != 0>), grid,
            dim3(256), 0, s, (bf16*)c, (float*)ws, (const bf16*)x, (const uint8_t*)wp, (const void*)scale, M, N, K,
            p.kts);
      });
    });
  });
  DLLM_HIP_CHECK(hipGetLastError());
  if (p.S > 1) {
    const size_t mn4 = (size_t)M * N / 4;
    hipLaunchKernelGGL(w4_reduce_kernel, dim3((unsigned)((mn4 + 255) / 256)), dim3(256), 0, s, (bf16*)c,
                       (const float*)ws, p.S, mn4);
    DLLM_HIP_CHECK(hipGetLastError());
  }
  return p.S;
}

void dequant_w4(uintptr_t out, uintptr_t wp, uintptr_t scale, int N, int K, int zp, uintptr_t stream) {
  DLLM_HOST_CHECK(N >= QBN && N % QBN == 0 && K >= QG && K % QG == 0, "N % 128 and K % 128");
  DLLM_HOST_CHECK(out != 0 && wp != 0 && scale != 0, "null operand");
  const size_t nblk = (size_t)(N / 16) * (K / QG);
  dispatch_value<0, 1>(zp != 0, "dequant_w4: zero points", [&](auto z) {
    hipLaunchKernelGGL(dequant_w4_kernel<decltype(z)::value != 0>, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), (bf16*)out, (const uint32_t*)wp, (const void*)scale, K,
                       nblk);
  });
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
