// Host-side helpers shared by the launchers: picking template arguments from runtime values, and the
// K split of the tiled GEMMs (gemm_wide, gemm_wide_fp8, gemm_pp, gemm_sq).  No device code.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"
#include "launchers.h"

namespace dllm {

// f(std::integral_constant<int, V>{}) for the one V of Vs that equals v: a runtime value picks a template
// argument (a bool: dispatch_value<0, 1>)
template <int... Vs, typename F>
static void dispatch_value(int v, const char* what, F&& f) {
  if (!((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...)) throw std::runtime_error(what);
}

// A launcher's K split: `splits` slices asked for over K / ktile K-tiles -> kts K-tiles per slice and the
// S slices that actually run (what the launcher returns; the slabs a deferred reduce must sum).
// mode 0: C = A B^T;  mode 1: SwiGLU;  mode 2: leave the S > 1 partial slabs in ws, no reduce.
struct SplitK {
  int kts, S;
};

static inline SplitK splitk_plan(int K, int ktile, int splits, int mode) {
  DLLM_HOST_CHECK(mode == 0 || mode == 1 || mode == 2, "mode");
  DLLM_HOST_CHECK(splits >= 1, "splits >= 1");
  const int ktiles = K / ktile;
  const int kts = (ktiles + splits - 1) / splits;
  const int S = (ktiles + kts - 1) / kts;
  DLLM_HOST_CHECK(mode != 2 || S > 1, "mode 2 needs a K split");
  return {kts, S};
}

// before the launch: S slabs of [M, N] fit the workspace
static inline void splitk_check_ws(const SplitK& p, uintptr_t ws, long ws_floats, int M, int N) {
  if (p.S > 1) DLLM_HOST_CHECK(ws != 0 && (long)p.S * M * N <= ws_floats, "split-K workspace too small");
}

// after the launch: the slabs stay (mode 2) or are summed into c (the SwiGLU of mode 1 applied there); -> S
static inline int splitk_finish(const SplitK& p, uintptr_t c, uintptr_t ws, int M, int N, int mode, uintptr_t stream) {
  DLLM_HIP_CHECK(hipGetLastError());
  if (p.S > 1 && mode != 2) splitk_reduce_ex(c, ws, 0, p.S, M, N, mode == 1 ? 1 : 0, stream);
  return p.S;
}

}  // namespace dllm
