// Schedule 2's K-tile of the 4-wave 256 x 256 MFMA kernels, shared by the persistent prefill GEMM
// (gemm_pf in gemm_pp.hip) and the fused LM-head log-likelihood kernel (lm_head_logprobs.hip): the
// LDS ring's swizzle, the counted waits, and the MFMA stream of one 64-deep K-tile with its fragment
// reads and LDS-DMA pieces in program order.  The design notes are at the head of gemm_pp.hip.
#pragma once
#include "common.h"

#include <type_traits>
#include <utility>

namespace dllm {

namespace {
constexpr int PBK = 64;                       // K per ring slot (128-byte rows)
typedef __attribute__((address_space(3))) void* lds_vptr_p;
typedef __attribute__((address_space(1))) void* glb_vptr_p;

__device__ __forceinline__ int pswz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

template <int OFF>
__device__ __forceinline__ bf16x8 pp_frag(uint32_t addr) {
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}

// s_waitcnt vmcnt(N) for a compile-time N
template <int N>
__device__ __forceinline__ void pp_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// f(integral_constant<int, i>) for i = 0 .. N-1, each i a constant expression
template <int... I, class F>
__device__ __forceinline__ void pp_static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void pp_static_for(F&& f) {
  pp_static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// s_waitcnt lgkmcnt(N) for a compile-time N (16 = no wait); a sched_barrier keeps hipcc from
// hoisting register-only MFMAs above an inline-asm wait (guide rule 18)
template <int N>
__device__ __forceinline__ void pp_lgkm() {
  static_assert(N >= 0 && N <= 16, "lgkmcnt");
  if constexpr (N < 16) {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
  }
}

// {barrier after set-1 reads (MFMA), barrier before set-0 reads, MFMAs between pieces (0 = spread
// over the rest of the K-tile), row tiles per group of the tile order}
struct PfSched {
  int ib1, ib3, ge, gm;
};
constexpr PfSched kPfSched{40, 88, 0, 8};

// The persistent kernels' K-tile for a wave tile of RT x CT 16 x 16 fragments, G LDS-DMA pieces per
// wave and K-tile, a ring of NB slots.  Fragment sets: (fa0, fb0) = K-half 0, (fa1, fb1) = K-half 1;
// a_off / b_off: byte offsets of the wave's A rows / B rows inside a slot.
template <int RT, int CT, int G, int NB>
struct PfKtile {
  static constexpr int NMF = RT * CT, NR = RT + CT;
  static constexpr PfSched SC = kPfSched;
  static constexpr int IB1 = SC.ib1;
  static constexpr int GE = SC.ge ? SC.ge : ((2 * NMF - 4 - IB1 - 1) / G > 1 ? (2 * NMF - 4 - IB1 - 1) / G : 1);
  static constexpr int IB3 = SC.ib3;
  static_assert(IB1 > 2 * NR - 1 && IB1 < NMF && IB3 >= NMF, "schedule 2 barriers");
  static constexpr int PB3 = (IB3 - IB1 - 1) / GE + 1 < G ? (IB3 - IB1 - 1) / GE + 1 : G;
  static constexpr int VC = (NB - 2) * G + PB3;
  static_assert(IB1 + 1 + GE * (G - 1) < 2 * NMF && IB3 + 1 + 2 * (NR - 1) < 2 * NMF, "schedule 2 fits a K-tile");
  static_assert(VC <= 63, "vmcnt");

  // read m of a fragment set: B fragments first, then A rows; the fragment's offset sits in the
  // instruction's immediate field
  template <int m>
  static __device__ __forceinline__ void rd(bf16x8 (&fa)[RT], bf16x8 (&fb)[CT], uint32_t base, uint32_t a_off,
                                            uint32_t b_off) {
    if constexpr (m < CT) fb[m] = pp_frag<m * 16 * 128>(base + b_off);
    else fa[m - CT] = pp_frag<(m - CT) * 16 * 128>(base + a_off);
  }

  // prologue: K-half 0 of the first K-tile (landed, barrier passed) into set 0
  static __device__ __forceinline__ void read_first(bf16x8 (&fa0)[RT], bf16x8 (&fb0)[CT], uint32_t base,
                                                    uint32_t a_off, uint32_t b_off) {
    pp_static_for<NR>([&](auto mc) { rd<decltype(mc)::value>(fa0, fb0, base, a_off, b_off); });
    __builtin_amdgcn_sched_barrier(0);
  }

  // One K-tile.  base1: this K-tile's slot + the lane's K-half 1 offset; base0: the next slot + the
  // K-half 0 offset; piece(p): stage piece p of the K-tile NB ahead into this K-tile's slot.
  // Set-1 reads from the start, barrier after MFMA IB1 (slot free), pieces one every GE MFMAs,
  // counted vmcnt + barrier after MFMA IB3 (next K-tile landed -- across a tile boundary too), then
  // the next K-half 0 reads into set 0.
  template <class Piece>
  static __device__ __forceinline__ void run(f32x4 (&acc)[RT][CT], bf16x8 (&fa0)[RT], bf16x8 (&fb0)[CT],
                                             bf16x8 (&fa1)[RT], bf16x8 (&fb1)[CT], uint32_t base0, uint32_t base1,
                                             uint32_t a_off, uint32_t b_off, Piece&& piece) {
    pp_static_for<2 * NMF>([&](auto ic) {
      constexpr int i = decltype(ic)::value, h = i / NMF, j = i % NMF, r = j / CT, c = j % CT;
      if constexpr (h == 0 && c == 0) {
        constexpr int w0 = (RT - 1 - r) + (j / 2 < NR ? j / 2 : NR);
        pp_lgkm<(w0 > 15 ? 15 : w0)>();
      }
      if constexpr (h == 0)
        acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb0[c], fa0[r], acc[r][c], 0, 0, 0);
      else
        acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb1[c], fa1[r], acc[r][c], 0, 0, 0);
      if constexpr (i % 2 == 1 && i / 2 < NR) rd<i / 2>(fa1, fb1, base1, a_off, b_off);
      if constexpr (i == IB1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
      if constexpr (i > IB1 && (i - IB1 - 1) % GE == 0 && (i - IB1 - 1) / GE < G) piece((i - IB1 - 1) / GE);
      if constexpr (i == IB3) {
        pp_vm<VC>();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
      if constexpr (i > IB3 && (i - IB3 - 1) % 2 == 0 && (i - IB3 - 1) / 2 < NR)
        rd<(i - IB3 - 1) / 2>(fa0, fb0, base0, a_off, b_off);
      __builtin_amdgcn_sched_barrier(0);
    });
  }
};
}  // namespace

}  // namespace dllm
