// w4_repack: an AWQ or GPTQ 4-bit projection, as its checkpoint stores it, into the fragment order of gemm_w4.hip
// -- a 4-bit transpose on the device (Llama-3-70B has 35 GB of codes; the host would need minutes and a second
// copy).  Formats (contract: ops/reference.py unpack_awq / unpack_gptq), group size 128, W the [N, K] weight:
//   AWQ "gemm":  qweight i32 [K, N / 8], nibble i of word [k, c] is W's row 8 c + (0,2,4,6,1,3,5,7)[i]: a word holds
//                eight ROWS of one k;  qzeros i32 [K / 128, N / 8] in the same order, the true zero
//   GPTQ:        qweight i32 [K / 8, N], nibble i of word [r, n] is k = 8 r + i: a word holds eight K of one row;
//                qzeros i32 [K / 128, N / 8] in natural order, zero - 1 (v1, mod 16) or the true zero (v2)
//   both:        scales f16 (or bf16) [K / 128, N]
// Output: the 1 KiB blocks (16-row tile t, group g) of ops/int4.py pack -- lane r + 16 q owns 16 bytes, word j =
// the eight k 32 j + 8 q + e of row r, code e at bit 4 (e / 2) + 16 (e % 2) -- and one dword per (row, group)
// [N / 16, K / 128, 16]: the scale's f32 bits | zero (gemm_w4.hip, "Zero-point variant").
//
// A workgroup (256 threads) owns 128 rows x one group = eight output blocks, 8 KiB in and 8 KiB out:
//  * phase 1 turns input words into output words in registers and puts them into LDS at their place in the
//    output blocks.  GPTQ: a thread takes eight words [16 g + r', n0 + n], 128 consecutive n (512 bytes) per row r';
//    its output word (row n, j = r' / 4, q = r' % 4) is the same eight codes with the nibbles reordered
//    (two mask-and-shift compressions).  AWQ: thread (c, j, q) takes the eight words [128 g + 32 j + 8 q + e, n0 / 8
//    + c], 16 consecutive c (64 bytes) per k, and transposes the 8 x 8 nibbles: output word i is nibble i of the
//    eight inputs, for row 8 c + order[i];
//  * LDS layout: word (tile t, q, r, j) at 272 t + 68 q + 4 r + j -- a lane's four words stay 16 bytes, and the
//    paddings spread phase 1's scattered word stores over 16 banks (4-way, against 32-way unpadded);
//  * phase 2: every thread reads two lanes' 16 bytes from LDS and stores them whole: a wave writes one 1 KiB block
//    per instruction;
//  * threads 0..127 build the 128 scale | zero dwords of the region.
// No atomics, every output byte is written exactly once, rows outside row0 .. row0 + N are not touched.
#include "common.h"
#include "launch_host.h"
#include "launchers.h"

namespace dllm {

namespace {
typedef uint32_t u32x4r __attribute__((ext_vector_type(4)));
constexpr int RROWS = 128, RG = 128;             // rows and k of a workgroup's region
constexpr int RTS = 272, RQS = 68;                // LDS words per tile, per q

// nibbles at bits 8 b (b = 0..3) of x -> bits 4 b
__device__ __forceinline__ uint32_t squeeze4(uint32_t x) {
  x = (x | (x >> 4)) & 0x00FF00FFu;
  return (x | (x >> 8)) & 0x0000FFFFu;
}
// eight codes in natural order (code e at bit 4 e) -> the fragment word (code e at bit 4 (e / 2) + 16 (e % 2))
__device__ __forceinline__ uint32_t frag_word(uint32_t w) {
  return squeeze4(w & 0x0F0F0F0Fu) | (squeeze4((w >> 4) & 0x0F0F0F0Fu) << 16);
}
}  // namespace

// FMT 0: AWQ, 1: GPTQ v1 (zero - 1 stored), 2: GPTQ v2
template <int FMT, bool SBF16>
__global__ void __launch_bounds__(256) w4_repack_kernel(uint32_t* __restrict__ Wp, uint32_t* __restrict__ Sz,
                                                        const uint32_t* __restrict__ Qw,
                                                        const uint32_t* __restrict__ Qz,
                                                        const uint16_t* __restrict__ Sc, int N, int K, int row0) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[8 * RTS];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * RROWS, g = blockIdx.y;
  const int G = K / RG;

  if constexpr (FMT == 0) {
    const int c = tid & 15, q = (tid >> 4) & 3, j = tid >> 6;
    const uint32_t* src = Qw + (size_t)(g * RG + 32 * j + 8 * q) * (N / 8) + n0 / 8 + c;
    uint32_t in[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) in[e] = __builtin_nontemporal_load(src + (size_t)e * (N / 8));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint32_t o = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) o |= ((in[e] >> (4 * i)) & 15u) << (4 * (e >> 1) + 16 * (e & 1));
      const int r = 8 * (c & 1) + (((i & 3) << 1) | (i >> 2));        // row 8 c + order[i] of the region
      lds[(c >> 1) * RTS + q * RQS + r * 4 + j] = o;
    }
  } else {
    const int n = tid & 127;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int rp = 2 * it + (tid >> 7);                              // word row 16 g + rp: j = rp / 4, q = rp % 4
      const uint32_t w = __builtin_nontemporal_load(Qw + (size_t)(g * 16 + rp) * N + n0 + n);
      lds[(n >> 4) * RTS + (rp & 3) * RQS + (n & 15) * 4 + (rp >> 2)] = frag_word(w);
    }
  }

  if (tid < RROWS) {
    const int n = n0 + tid;
    const uint32_t zw = Qz[(size_t)g * (N / 8) + n / 8];
    const int m = n & 7;
    uint32_t z;
    if constexpr (FMT == 0) z = (zw >> (4 * ((m >> 1) | ((m & 1) << 2)))) & 15u;      // the slot i with order[i] = m
    else z = ((zw >> (4 * m)) + (FMT == 1 ? 1u : 0u)) & 15u;
    const uint16_t sb = Sc[(size_t)g * N + n];
    float s;
    if constexpr (SBF16) s = __uint_as_float((uint32_t)sb << 16);
    else s = (float)__builtin_bit_cast(_Float16, sb);
    Sz[((size_t)((row0 + n) >> 4) * G + g) * 16 + (n & 15)] = (__float_as_uint(s) & ~15u) | z;
  }
  __syncthreads();

  const int lane = tid & 63;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int t = (tid >> 6) + 4 * it;
    const u32x4r v = *reinterpret_cast<const u32x4r*>(lds + t * RTS + (lane >> 4) * RQS + (lane & 15) * 4);
    const size_t blk = (size_t)((row0 + n0) / 16 + t) * G + g;
    reinterpret_cast<u32x4r*>(Wp + blk * 256)[lane] = v;
  }
}

void w4_repack(uintptr_t wp, uintptr_t sz, uintptr_t qweight, uintptr_t qzeros, uintptr_t scales, int fmt,
               int scale_bf16, int N, int K, int dstN, int row0, uintptr_t stream) {
  DLLM_HOST_CHECK(N >= RROWS && N % RROWS == 0 && K >= RG && K % RG == 0, "N % 128 and K % 128");
  DLLM_HOST_CHECK(row0 >= 0 && row0 % 16 == 0 && dstN % 128 == 0 && (long)row0 + N <= dstN, "rows row0 .. row0 + N of dstN");
  DLLM_HOST_CHECK(K / RG <= 65535, "K groups");
  DLLM_HOST_CHECK(wp != 0 && sz != 0 && qweight != 0 && qzeros != 0 && scales != 0, "null operand");
  const dim3 grid(N / RROWS, K / RG);
  dispatch_value<0, 1, 2>(fmt, "w4_repack: format", [&](auto f) {
    dispatch_value<0, 1>(scale_bf16 != 0, "w4_repack: scale dtype", [&](auto b) {
      hipLaunchKernelGGL((w4_repack_kernel<decltype(f)::value, decltype(b)::value != 0>), grid, dim3(256), 0,
                         reinterpret_cast<hipStream_t>(stream), (uint32_t*)wp, (uint32_t*)sz, (const uint32_t*)qweight,
                         (const uint32_t*)qzeros, (const uint16_t*)scales, N, K, row0);
    });
  });
  DLLM_HIP_CHECK(hipGetLastError());
}

}  // namespace dllm
