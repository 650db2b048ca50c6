// Multi-LoRA: different adapters on different rows of one batch, as an additive delta after a
// projection's GEMM (contract: ops/reference.py lora_apply).  For a token row t with adapter slot a:
//   v[t, j] = bf16( sum_k x[t, k] * A_a[j, k] )              f32 accumulation, one rounding
//   d[t, n] = sum_j v[t, j] * B_a[n, j]                      f32
//   y[t, n] = bf16( f32(y[t, n]) + scale_a * d[t, n] )       one rounding, in place
//
// A packed projection (q|k|v, gate|up) holds `nslices` LoRA modules over one input: A is stacked to
// [slots][R = nslices * rp][K] (rp: the rank zero-padded to 32 or 64), B is [slots][N][rp] with row n
// taken from the module that owns output column n, and column n multiplies the v slice of its module
// (slice boundaries off1 / off2, multiples of 64; unused boundaries = N).
//
// ROW PLAN (host, once per step, ops/lora.py): token rows sorted stably by slot and cut into tiles of
// 16 rows of one slot: tile_slot [nt] (-1: an unused tile of a graph's static plan), tile_rows
// [nt * 16] (-1: padding).  Rows without an adapter are in no tile and are never touched.
//
//   lora_shrink  grid (nt, ksplit): a workgroup gathers its 16 rows of x and multiplies one K slice
//                (kKSlice columns) by the stacked A of its slot; f32 partials ws[ksplit][nt*16][R].
//                No atomics: the K slices are summed by the consumer in slice order.
//   lora_expand  grid (nt, column blocks of 256): sums the partials in slice order, rounds to bf16
//                once (v), multiplies by the B rows of its columns and updates y in place.  The B tile
//                is the MFMA's A operand and v^T its B operand, so a lane's four accumulator registers
//                are four consecutive output columns of one token row; a wave's four MFMAs take the B
//                rows of its 64 columns in an order that gives a lane two runs of 8 consecutive
//                columns: 16-byte read-modify-writes, 64 contiguous bytes per row and access.
//
// mfma_f32_16x16x32_bf16 maps (lane l, g = l >> 4): A[row l & 15][k = 8 g + j], B[k = 8 g + j][col l & 15],
// C/D[row 4 g + reg][col l & 15].
#include "common.h"
#include "launchers.h"

#pragma clang fp contract(off)

namespace dllm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DLLM_WAVE;
constexpr int kTile = 16;           // rows of a tile = the MFMA's M / N
constexpr int kKSlice = 512;        // x columns one shrink workgroup reduces
constexpr int kMaxNB = 3;           // 16-column blocks of R per wave: R <= 16 * kMaxNB * kWaves = 192
constexpr int kGroup = 64;          // output columns of one expand wave: four MFMAs
constexpr int kColBlock = kGroup * kWaves;      // output columns of one expand workgroup
constexpr int kMaxRp = 64;

__global__ __launch_bounds__(kThreads) void lora_shrink_kernel(
    float* __restrict__ ws, const bf16* __restrict__ x, const bf16* __restrict__ A,
    const int32_t* __restrict__ tile_slot, const int32_t* __restrict__ tile_rows, int T, int K, int R, int nslots,
    int nt) {
  const int tile = blockIdx.x, ks = blockIdx.y;
  const int slot = tile_slot[tile];
  if (slot < 0 || slot >= nslots) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int nblocks = R / kTile;
  if (wave >= nblocks) return;
  const int row = tile_rows[tile * kTile + l15];
  const bool live = row >= 0 && row < T;
  const int k0 = ks * kKSlice, k1 = min(K, k0 + kKSlice);
  const bf16* xr = x + (size_t)(live ? row : 0) * K + 8 * g;
  const bf16* Ar = A + ((size_t)slot * R + l15) * K + 8 * g;
  f32x4 acc[kMaxNB];
#pragma unroll
  for (int i = 0; i < kMaxNB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero = {};
#pragma unroll 2
  for (int k = k0; k < k1; k += 32) {
    const bf16x8 xa = live ? *reinterpret_cast<const bf16x8*>(xr + k) : zero;
#pragma unroll
    for (int i = 0; i < kMaxNB; ++i) {
      const int nb = wave + i * kWaves;
      if (nb < nblocks) {
        const bf16x8 ab = *reinterpret_cast<const bf16x8*>(Ar + (size_t)nb * kTile * K + k);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa, ab, acc[i], 0, 0, 0);
      }
    }
  }
  // C[token row 4 g + reg][col l15] of block nb
  float* out = ws + ((size_t)ks * nt * kTile + (size_t)tile * kTile) * R;
#pragma unroll
  for (int i = 0; i < kMaxNB; ++i) {
    const int nb = wave + i * kWaves;
    if (nb < nblocks) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(4 * g + r) * R + nb * kTile + l15] = acc[i][r];
    }
  }
}

__global__ __launch_bounds__(kThreads) void lora_expand_kernel(
    bf16* __restrict__ y, long ldy, const float* __restrict__ ws, const bf16* __restrict__ B,
    const float* __restrict__ scale, const int32_t* __restrict__ tile_slot, const int32_t* __restrict__ tile_rows,
    int T, int N, int R, int rp, int off1, int off2, int ksplit, int nslots, int nt) {
  const int tile = blockIdx.x;
  const int slot = tile_slot[tile];
  if (slot < 0 || slot >= nslots) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int row = tile_rows[tile * kTile + l15];
  const bool live = row >= 0 && row < T;
  const float sc = scale[slot];
  const int ksteps = rp / 32;
  const size_t slab = (size_t)nt * kTile * R;
  const float* wrow = ws + ((size_t)tile * kTile + l15) * R + 8 * g;
  // One 64-column group per wave.  The group's B rows are handed to four MFMAs in an order that leaves
  // lane group g with columns c0 .. c0 + 7 and c0 + 32 .. c0 + 39 (c0 = n0 + 8 g) of its token row: MFMA i
  // takes, as its row 4 g' + r', B row n0 + 32 (i >> 1) + 8 g' + 4 (i & 1) + r', so its accumulator
  // register reg of lane group g is column n0 + 32 (i >> 1) + 8 g + 4 (i & 1) + reg.  A lane then
  // updates y in two 16-byte pieces and a wave 64 contiguous bytes of each of its 16 rows per access.
  const int n0 = blockIdx.y * kColBlock + wave * kGroup;
  if (n0 >= N) return;
  const int slice = (n0 >= off1) + (n0 >= off2);       // slice boundaries are multiples of kGroup
  // v^T fragment: v[token l15][slice * rp + 32 s + 8 g + j], the partials summed in slice order
  bf16x8 vf[kMaxRp / 32];
#pragma unroll
  for (int s = 0; s < kMaxRp / 32; ++s) {
    if (s < ksteps) {
      float a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = 0.f;
      const float* p = wrow + slice * rp + 32 * s;
      for (int q = 0; q < ksplit; ++q) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p + q * slab);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(p + q * slab + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] += lo[j];
          a[4 + j] += hi[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[s][j] = f2bf(a[j]);
    }
  }
  f32x4 acc[4];
  const bf16x8 zero = {};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int brow = n0 + 32 * (i >> 1) + 8 * (l15 >> 2) + 4 * (i & 1) + (l15 & 3);
    const bf16* br = B + ((size_t)slot * N + (brow < N ? brow : 0)) * rp + 8 * g;
#pragma unroll
    for (int s = 0; s < kMaxRp / 32; ++s) {
      if (s < ksteps) {
        const bf16x8 bw = brow < N ? *reinterpret_cast<const bf16x8*>(br + 32 * s) : zero;
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw, vf[s], acc[i], 0, 0, 0);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c0 = n0 + 32 * h + 8 * g;                // N is a multiple of 16: the 8 columns are all in or all out
    if (c0 < N) {
      bf16x8* yp = reinterpret_cast<bf16x8*>(y + (size_t)row * ldy + c0);
      bf16x8 o = *yp;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dlt = sc * acc[2 * h + (e >> 2)][e & 3];
        o[e] = f2bf(bf2f(o[e]) + dlt);
      }
      *yp = o;
    }
  }
}

}  // namespace

int lora_ksplit(int K) { return (K + kKSlice - 1) / kKSlice; }

void lora_shrink(uintptr_t ws, long ws_floats, uintptr_t x, uintptr_t A, uintptr_t tile_slot, uintptr_t tile_rows,
                 int T, int K, int R, int nslots, int nt, uintptr_t stream) {
  DLLM_HOST_CHECK(T >= 0 && nt >= 0 && nslots >= 1, "lora_shrink: sizes");
  DLLM_HOST_CHECK(K >= 32 && K % 32 == 0, "lora_shrink: K must be a multiple of 32");
  DLLM_HOST_CHECK(R >= kTile && R % kTile == 0 && R <= kTile * kMaxNB * kWaves, "lora_shrink: stacked rank");
  const int ksplit = lora_ksplit(K);
  DLLM_HOST_CHECK(ws_floats >= (long)ksplit * nt * kTile * R, "lora_shrink: workspace too small");
  DLLM_HOST_CHECK(ksplit <= 65535, "lora_shrink: K too large");
  if (nt == 0) return;
  hipLaunchKernelGGL(lora_shrink_kernel, dim3(nt, ksplit), dim3(kThreads), 0, (hipStream_t)stream, (float*)ws,
                     (const bf16*)x, (const bf16*)A, (const int32_t*)tile_slot, (const int32_t*)tile_rows, T, K, R,
                     nslots, nt);
  DLLM_HIP_CHECK(hipGetLastError());
}

void lora_expand(uintptr_t y, long ldy, uintptr_t ws, long ws_floats, uintptr_t B, uintptr_t scale,
                 uintptr_t tile_slot, uintptr_t tile_rows, int T, int N, int K, int R, int rp, int off1, int off2,
                 int nslots, int nt, uintptr_t stream) {
  DLLM_HOST_CHECK(T >= 0 && nt >= 0 && nslots >= 1, "lora_expand: sizes");
  DLLM_HOST_CHECK(rp == 32 || rp == 64, "lora_expand: padded rank must be 32 or 64");
  DLLM_HOST_CHECK(R % rp == 0 && R / rp >= 1 && R / rp <= 3, "lora_expand: 1 to 3 slices");
  DLLM_HOST_CHECK(N >= kTile && N % kTile == 0 && ldy >= N && ldy % 8 == 0 && y % 16 == 0,
                  "lora_expand: N a multiple of 16, rows 16-byte aligned");
  DLLM_HOST_CHECK((off1 % kGroup == 0 || off1 == N) && (off2 % kGroup == 0 || off2 == N) && 0 < off1 &&
                      off1 <= off2 && off2 <= N,
                  "lora_expand: slice boundaries must be multiples of 64");
  // the slices the boundaries name must exist in the stacked v
  DLLM_HOST_CHECK((off1 >= N || R / rp >= 2) && (off2 >= N || R / rp >= 3), "lora_expand: more boundaries than slices");
  const int ksplit = lora_ksplit(K);
  DLLM_HOST_CHECK(ws_floats >= (long)ksplit * nt * kTile * R, "lora_expand: workspace too small");
  const int cblocks = (N + kColBlock - 1) / kColBlock;
  DLLM_HOST_CHECK(cblocks <= 65535, "lora_expand: N too large");
  if (nt == 0) return;
  hipLaunchKernelGGL(lora_expand_kernel, dim3(nt, cblocks), dim3(kThreads), 0, (hipStream_t)stream, (bf16*)y, ldy,
                     (const float*)ws, (const bf16*)B, (const float*)scale, (const int32_t*)tile_slot,
                     (const int32_t*)tile_rows, T, N, R, rp, off1, off2, ksplit, nslots, nt);
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
