"""Dense GEMM host path for y = x @ w^T (w is [N, K], nn.Linear layout): :func:`route` decides which
hand-written gfx950 kernel runs, with how many K slices and which variant word; one launch helper runs
it.  The route is an ordered list -- the first branch that takes the call wins; every cutover is a field
of :mod:`..knobs`, measured in the engine on Llama-3-8B / 70B shapes.  ``linear``:

1. decode LM head (N > 65536, knobs.pp_head_min_m <= M <= 256) on gemm_pp schedule 2, unsplit, weights
   nontemporal: 236 vs 268 us for gemm_sq at M = 256 -- unless comm kernels may hold CUs: beside a
   4-workgroup, 20 KiB-LDS receive spinning in another process it took 284 us, gemm_sq 268 either way
   (bench/debug/lm_head_bench.py, profiles/round5_raw/r5ae_head.txt; knobs.head_beside_comm);
2. long-K decode down projection (K >= knobs.pp_down_min_k, 225 <= M <= 256; 70B: K = 28672) on gemm_pp's
   128-column tile, K slices filling the CUs, weights nontemporal: 126 vs 135 us for gemm_wide
   (bench/debug/medium_m_sweep.py, profiles/round6_gate_up_pp.md); not beside comm kernels;
3. gemm_wide's decode ranges (64/128/192/256-row x 128 tiles, 3-stage LDS-DMA pipeline, split-K over
   workgroups; profiles/wide_gemm.md): down (K >= 8192 and K > N) to knobs.wide_down_max_m, the
   o-projection (N <= K) to wide_o_max_m, qkv / LM head to wide_proj_max_m; small weights (N K <=
   knobs.wide_small_bm_maxw: the 8B o-projection) on 128-row tiles with half the K slices.  Inside the
   range gemm_sq's 256 x 256 tile -- a third fewer staged bytes per FLOP -- takes knobs.sq_min_m (225: at
   192 it loses 1-6 %) <= M <= 256 where its grid needs no K split (:func:`use_sq`): LM head 1.05x, 70B
   gate|up 1.07x; split grids lose 6-20 % to the slab traffic (knobs.sq roles; knobs.sq_split admits them);
4. M >= knobs.pp_proj_min_m: the persistent 256 x 256 schedule-2 kernel (gemm_pf in gemm_pp.hip,
   knobs.pp_persistent) where its grid fills the chip (:func:`pf_fills`), else split-K gemm_pp -- medium
   M, mixed steps, short prompts (profiles/round4_gemm_counters.md, profiles/round5_medium_m_gemm.md);
5. what none takes (a bias, N % 256 above the decode range, fp32, operands >= 4 GiB): torch's F.linear.

``linear_swiglu`` (w = [Wg; Wu], the SwiGLU in the epilogue):
1. decode gate|up at knobs.pp_gate_up_min_m (200) <= M <= 256 on gemm_pp, unsplit, weights nontemporal, on
   the column tile (128, else 256) that gives one round of CUs / 2 .. CUs tiles: 8B (224 x 128 columns)
   62.1 vs 64.1 us for gemm_wide, 70B (224 x 256 columns) 204 vs 259 us for gemm_sq
   (bench/debug/medium_m_sweep.py --pp, profiles/round6_gate_up_pp.md); not beside comm kernels;
2. gemm_wide to knobs.wide_gate_up_max_m, gemm_sq on its unsplit grids as above;
3. M >= knobs.pp_swiglu_min_m: gemm_pf where it fills the chip, else gemm_pp;
4. no fused kernel: the plain product's route, marked ``unfused`` (silu_mul follows).
The role is inferred from the shape: "down" = K >= 8192 and K > N, so the square / widening K = 8192
projections of 70B-class models (qkv 8192 -> 10240, o 8192 -> 8192) stay "proj".
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from .. import _ext
from .. import knobs

# Variant words of the launchers.  Their numeric values are those of the recorded route table
# (tests/golden/gemm_routes.json); a launcher refuses a word whose kernel was retired (profiles/gemm_variants.md).
# gemm_pp: 128-column tile (else 256), weights nontemporal, grouped row-tile order (large M, no K split), schedule 2
# (every route sets it; schedule 1 stays as the tests' second implementation); bit 3 with PP_SCHED2: the profile build
# of bench/pp_timeline.py
PP_BN128, PP_NT, PP_GROUPED, PP_SCHED2 = 1, 2, 4, 64
PP_PREFILL_VARIANT = PP_SCHED2 | PP_GROUPED           # medium M and prefill: 256-column tile
PP_GATE_UP_VARIANT = PP_SCHED2 | PP_NT | PP_BN128     # decode gate|up (& ~PP_BN128: the 256-column form)
PP_HEAD_VARIANT = PP_SCHED2 | PP_NT                   # decode LM head (weights read once per step)
PP_DOWN_VARIANT = PP_SCHED2 | PP_NT | PP_BN128        # long-K decode down projection, split
# gemm_wide: bit 0 is set in every routed word (staging pieces between the MFMAs, weights nontemporal exactly on
# unsplit grids; word 0, pieces after the barrier, stays for the tests), WIDE_SPLITRD adds per-row
# fragment waits (unsplit grids: 27,123 vs 27,014 / 26,896 tok/s in the engine); from bit 8 (gemm_wide_fp8 too) a
# row-tile override (64 / 128 / 192 / 256; 0 = wide_bm(M))
WIDE_SPLITRD, WIDE_ROW_TILE_SHIFT = 32, 8
WIDE_VARIANT = 1 | WIDE_SPLITRD                # unsplit grids
WIDE_SPLIT_VARIANT = 1                         # split-K grids
SQ_VARIANT = 4                                 # gemm_sq's one word (staging pieces right after the barrier)
FP8_NT, FP8_CACHED, FP8_GROUPED = 1, 4, 64     # gemm_wide_fp8: weights nontemporal on unsplit grids / never; grouped order
PF_NT_STORES, PF_DYNAMIC = 8, 16               # gemm_pf: nontemporal output stores; per-XCD dynamic tile queues (DYN)


def is_down_proj(n: int, k: int) -> bool:
    """The MLP down projection's shape: long, narrowing K (8B: 14336 -> 4096, 70B: 28672 -> 8192).
    A K = 8192 qkv or o projection of a 70B-class model (N >= K) is not one."""
    return k >= 8192 and k > n


def _cus(device) -> int:
    n = _CUS.get(device)
    if n is None:                      # off the GPU: an MI355X's 256 (dispatch unit tests on CPU)
        d = torch.device(device)
        n = torch.cuda.get_device_properties(d.index or 0).multi_processor_count if d.type == "cuda" else 256
        _CUS[device] = n
    return n


_CUS = {}


def pf_fills(m: int, n: int, device=None, cus: int = 0) -> bool:
    """gemm_pf (one 256 x 256 tile per CU per round, no split-K) only where its grid fills the chip:
    at least one tile per CU and rounds that are mostly full (knobs.pf_min_eff), or many rounds.
    Below that the split-K gemm_pp grid wins at every measured M from 320 to 2048 -- gemm_pf's
    single-round grids run one tile's whole K loop: 74-78 us for the 8B o-projection at any
    M <= 2048, the down projection 250-283 us vs 55-174 us split (profiles/round5_medium_m_gemm.md)."""
    cus = cus or _cus(device)
    tiles = (-(-m // 256)) * (n // 256)
    if tiles < cus:
        return False
    rounds = -(-tiles // cus)
    return rounds >= 4 or tiles / (rounds * cus) >= knobs.K.pf_min_eff


def _bf16(x, w) -> bool:
    return x.dtype == w.dtype == torch.bfloat16 and x.is_contiguous() and w.is_contiguous()


def _use_wide(m: int, n: int, k: int, x=None, w=None, swiglu: bool = False) -> bool:
    """The decode ranges of gemm_wide (and, inside them, gemm_sq), per role (``x``, ``w``: eligible operands)."""
    kn = knobs.K
    roles = {t for t in kn.wide.split(",") if t and t != "none"}
    if not roles or m < 1 or n % 128 or k % 64 or not (x is None or _bf16(x, w)):
        return False
    down = is_down_proj(n, k) and not swiglu
    if "all" in roles:
        return m <= 512 or (down and m <= kn.wide_down_max_m)
    if "auto" in roles:
        if swiglu:
            return m <= kn.wide_gate_up_max_m
        if down:
            return m <= kn.wide_down_max_m
        return m <= (kn.wide_o_max_m if n <= k else kn.wide_proj_max_m)
    if swiglu:
        return "gate_up" in roles and m <= 512
    return ("down" in roles) if is_down_proj(n, k) else ("proj" in roles and m <= 512)


def _use_pp(m: int, n: int, k: int, x=None, w=None, min_m: int = 1) -> bool:
    """What gemm_pp / gemm_pf take from ``min_m`` rows: 256-column tiles, operands below 4 GiB (and eligible)."""
    return (0 < min_m <= m and n % 256 == 0 and k % 64 == 0 and m * k * 2 < (1 << 32) and n * k * 2 < (1 << 32)
            and (x is None or _bf16(x, w)))


class SplitKPartial:
    """Split-K partial sums of ``x @ w.T`` still in the per-stream workspace (not reduced).  Each K
    slice accumulates in f32; the slabs hold it as f16 x 2^-6 by default (csrc/kernels/common.h
    ``DLLM_PART_TYPE``: half the bytes of f32 slabs, 3 significand bits more than the bf16 result).

    Returned by ``linear(..., defer=True)`` when the split-K tiled kernel ran, so the NEXT op can
    fuse the reduction (``ops.fused_add_rms_norm`` -> splitk_add_rms_norm); anything else calls
    :meth:`materialize`.  Valid only until the next tiled GEMM on the same stream reuses the
    workspace -- consume it immediately."""

    __slots__ = ("ws", "splits", "m", "n", "shape", "dtype", "device")

    def __init__(self, ws, splits, m, n, shape, dtype, device):
        self.ws, self.splits, self.m, self.n = ws, splits, m, n
        self.shape, self.dtype, self.device = shape, dtype, device

    def materialize(self) -> torch.Tensor:
        y = torch.empty(self.shape, dtype=self.dtype, device=self.device)
        _ext.kernels().splitk_reduce(y.data_ptr(), self.ws.data_ptr(), 0, self.splits, self.m, self.n,
                                     torch.cuda.current_stream().cuda_stream)
        return y


class GemmRoute(NamedTuple):
    """What one dense GEMM call runs (immutable).  ``kernel``: "wide", "sq", "pp", "pf" or "torch" (F.linear);
    ``splits``: the K slices handed to the launcher, after the workspace clamp (0: the kernel takes none);
    ``variant``: the launcher's variant word, row-tile bits included; ``swiglu``: the SwiGLU runs in its epilogue;
    ``unfused``: a SwiGLU was asked for and no fused kernel takes it -- the plain product's route, silu_mul follows."""
    kernel: str
    splits: int = 0
    variant: int = 0
    swiglu: bool = False
    unfused: bool = False


def route(m: int, n: int, k: int, swiglu: bool = False, bias: bool = False, bf16: bool = True, cus: int = 256,
          comm_cus: Optional[int] = None) -> GemmRoute:
    """The route of ``x [M, K] @ w [N, K]^T`` (``swiglu``: w = [Wg; Wu], the SwiGLU fused).  Pure: shapes,
    ``bias`` (there is one), ``bf16`` (both operands bf16 and contiguous), the CU count, the CUs reserved for
    comm kernels (None: the current reservation) and knobs in.  The numbers are the module docstring's."""
    kn = knobs.K
    comm = _comm_cus if comm_cus is None else comm_cus
    if swiglu and bf16:
        # swiglu 1: decode gate|up on gemm_pp, one round of CUs / 2 .. CUs tiles of 128, else 256 columns
        if 0 < kn.pp_gate_up_min_m <= m <= 256 and not comm and _use_pp(m, n, k):
            if n % 128 == 0 and cus // 2 <= n // 128 <= cus:
                return GemmRoute("pp", 1, PP_GATE_UP_VARIANT, True)
            if cus // 2 <= n // 256 <= cus:
                return GemmRoute("pp", 1, PP_GATE_UP_VARIANT & ~PP_BN128, True)
        if _use_wide(m, n, k, swiglu=True):                              # swiglu 2: gemm_wide, or gemm_sq unsplit
            return _sq_route(m, n, k, True) if use_sq(m, n, k, True) else _wide_route(m, n, k, True, comm_cus=comm)
        if _use_pp(m, n, k, min_m=kn.pp_swiglu_min_m):                   # swiglu 3: gemm_pf where it fills, else gemm_pp
            if kn.pp_persistent and m * (n // 2) * 2 < (1 << 31) and pf_fills(m, n, cus=cus):
                return _pf_route(k, True, comm_cus=comm)
            return _pp_route(m, n, k, True, variant=PP_PREFILL_VARIANT)
    if swiglu:                                                           # swiglu 4: unfused, the plain product's route
        return route(m, n, k, False, bias, bf16, cus, comm)._replace(unfused=True)
    if bias or not bf16:                                                 # linear 5
        return GemmRoute("torch")
    if n > 65536 and 0 < kn.pp_head_min_m <= m <= 256 and (not comm or kn.head_beside_comm == "pp") \
            and _use_pp(m, n, k):
        return GemmRoute("pp", 1, PP_HEAD_VARIANT)                       # linear 1: decode LM head on gemm_pp
    if 0 < kn.pp_down_min_k <= k and 225 <= m <= 256 and is_down_proj(n, k) and not comm and n % 128 == 0 \
            and _use_pp(m, n, k):                                        # linear 2: long-K down on split gemm_pp
        return _pp_route(m, n, k, False, max(1, min(16, cus // (n // 128))), PP_DOWN_VARIANT)
    if _use_wide(m, n, k):                                               # linear 3: gemm_wide, or gemm_sq unsplit
        return _sq_route(m, n, k, False) if use_sq(m, n, k) else _wide_route(m, n, k, False, comm_cus=comm)
    if _use_pp(m, n, k, min_m=kn.pp_proj_min_m):                         # linear 4: gemm_pf where it fills, else gemm_pp
        if kn.pp_persistent and m * n * 2 < (1 << 31) and pf_fills(m, n, cus=cus):
            return _pf_route(k, False, comm_cus=comm)
        return _pp_route(m, n, k, False, variant=PP_PREFILL_VARIANT)
    return GemmRoute("torch")                                            # linear 5


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, defer: bool = False):
    """y = x w^T (+bias).  ``defer``: may return a :class:`SplitKPartial` (see there)."""
    k = x.shape[-1]
    if w.shape[1] != k:
        raise ValueError(f"linear: x[..., {k}] vs w {tuple(w.shape)}")
    r = route(x.numel() // k, w.shape[0], k, False, bias is not None, _bf16(x, w), _cus(x.device))
    return F.linear(x, w, bias) if r.kernel == "torch" else _launch("gemm_" + r.kernel, x, w, r, defer)


def linear_swiglu(x: torch.Tensor, w_gate_up: torch.Tensor) -> Optional[torch.Tensor]:
    """silu(x Wg^T) * (x Wu^T) with W = [Wg; Wu] in one launch; None if the route is unfused."""
    k = x.shape[-1]
    r = route(x.numel() // k, w_gate_up.shape[0], k, True, False, _bf16(x, w_gate_up), _cus(x.device))
    return None if r.unfused else _launch("gemm_" + r.kernel, x, w_gate_up, r)


_ws = {}
_WS_FLOATS = 32 << 20          # 128 MiB of split-K partials per (device, stream)


def _workspace(device: torch.device, stream: Optional[int] = None) -> torch.Tensor:
    key = (device.index or 0, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    t = _ws.get(key)
    if t is None:
        t = _ws[key] = torch.empty(_WS_FLOATS, dtype=torch.float32, device=device)
    return t


def ws_splits(s: int, m: int, n: int) -> int:       # ``s`` K slices, or as many [M, N] slabs as the workspace holds
    return max(1, _WS_FLOATS // (m * n)) if s > 1 and s * m * n > _WS_FLOATS else s


def _launch(kernel: str, x, w, r: GemmRoute, defer: bool = False, scales=None):
    """Run launcher ``kernel`` as route ``r`` says: the workspace, mode 0 (plain) / 1 (SwiGLU) / 2 (``defer`` and
    a K split: the slabs stay in the workspace, returned as a :class:`SplitKPartial`), the output.  The route's
    maker has checked operands and tiles (route's predicates, _mnk, linear_fp8).  ``scales``: gemm_wide_fp8's
    quantized activation (q [M, K], scale [M]) -- ``x`` then only gives the result's shape and dtype."""
    k = x.shape[-1]
    n = w.shape[0]
    if scales is None:
        m = x.numel() // k
        ptrs = (x.data_ptr(), w.data_ptr())
    else:
        m = scales[0].shape[0]
        ptrs = (scales[0].data_ptr(), scales[1].data_ptr(), w.q.data_ptr(), w.scale.data_ptr())
    kern = getattr(_ext.kernels(), kernel)
    stream = torch.cuda.current_stream().cuda_stream
    mode = 2 if defer and not r.swiglu and r.splits > 1 else int(r.swiglu)
    y = None if mode == 2 else torch.empty(*x.shape[:-1], n // 2 if r.swiglu else n, dtype=x.dtype, device=x.device)
    if kernel == "gemm_pf":
        v = r.variant
        if v & PF_DYNAMIC and torch.cuda.is_current_stream_capturing():
            # inside a graph: the static tile walk.  A tile queue is per stream and self-resetting, but
            # a replay may run on another stream beside eager launches that use the same queue
            v &= ~PF_DYNAMIC
        kern(y.data_ptr(), *ptrs, m, n, k, mode, v, stream)
        return y
    ws = _workspace(x.device, stream)
    se = kern(0 if y is None else y.data_ptr(), *ptrs, ws.data_ptr(), ws.numel(), m, n, k, r.splits, mode, r.variant, stream)
    return SplitKPartial(ws, se, m, n, (*x.shape[:-1], n), x.dtype, x.device) if y is None else y


def _mnk(name: str, x, w, bn: int):
    """(M, N, K) of a direct ``linear_*`` call, after the operand and tile checks."""
    k = x.shape[-1]
    if not _bf16(x, w):
        raise ValueError(f"{name}: bf16 contiguous operands")
    if w.shape[0] % bn or k % 64:
        raise ValueError(f"{name}: N % {bn} and K % 64")
    return x.numel() // k, w.shape[0], k


def wide_bm(m: int) -> int:
    """Row tile of gemm_wide for M rows (mirrors wide_bm in csrc/kernels/gemm_wide.hip)."""
    for bm in (64, 128, 192, 256):
        if m <= bm:
            return bm
    return 192 if m <= 384 else 256


def wide_row_tile(m: int, n: int, k: int, swiglu: bool = False) -> int:
    """Row tile gemm_wide uses for this shape (knobs.wide_small_bm for small split grids, else
    wide_bm): e.g. 128 runs an M = 256 o-projection as 2 row tiles x 4 K slices instead of 1 x 8."""
    kn = knobs.K
    if kn.wide_small_bm and not swiglu and n * k <= kn.wide_small_bm_maxw and kn.wide_small_bm < wide_bm(m):
        return kn.wide_small_bm
    return wide_bm(m)


# CUs a co-resident communication kernel may hold (set by the RCCL transport of a pipeline stage:
# a p2p receive spins on its CUs for as long as its peer has not sent).  gemm_wide's split-K grids
# are sized to leave them free: its workgroups (144 KiB of LDS) cannot share a CU with a kernel
# holding LDS, so a 256-workgroup grid beside 4 such CUs runs a second round for 4 workgroups --
# the down projection took 1.58x its solo time beside a 4-CU receive, the 224 / 240-workgroup
# grids 1.00x (scripts/hwq_probe.py gemms, profiles/round5_comm_queues.md)
_comm_cus = 0
_comm_users = 0


def comm_cus() -> int:
    """The CUs currently reserved for comm kernels (0: none live)."""
    return _comm_cus


def pf_dynamic(comm_cus: Optional[int] = None) -> bool:
    """gemm_pf's dynamic tile queue: knobs.pf_dynamic "on" / "off" / "auto" (on while comm kernels may hold CUs)."""
    v = str(knobs.K.pf_dynamic).strip().lower()
    if v == "auto":
        return (_comm_cus if comm_cus is None else comm_cus) > 0
    return v in ("1", "true", "on", "yes")


def reserve_cus_for_comm(n: int) -> None:
    """A transport with spinning comm kernels starts: size gemm_wide grids around ``n`` CUs."""
    global _comm_cus, _comm_users
    _comm_users += 1
    _comm_cus = max(_comm_cus, int(n))


def release_cus_for_comm() -> None:
    global _comm_cus, _comm_users
    _comm_users = max(0, _comm_users - 1)
    if not _comm_users:
        _comm_cus = 0


def wide_splits(m: int, n: int, k: int, swiglu: bool = False, target_wgs: int = 0,
                comm_cus: Optional[int] = None, bm: int = 0) -> int:
    """K slices for gemm_wide: about one workgroup per CU, >= 8 K-tiles (512) per slice (with CUs
    reserved for communication: at most one workgroup per remaining CU).  ``bm``: the row tile, if known."""
    tiles = (n // 128) * (-(-m // (bm or wide_row_tile(m, n, k, swiglu))))
    target = target_wgs or knobs.K.wide_target_wgs
    comm = _comm_cus if comm_cus is None else comm_cus
    s = (target - comm) // tiles if comm else round(target / tiles)
    return max(1, min(s, (k // 64) // 8, 16))


def _wide_route(m, n, k, swiglu, splits=0, variant=-1, comm_cus=None) -> GemmRoute:
    bm = wide_row_tile(m, n, k, swiglu)
    s = ws_splits(splits or wide_splits(m, n, k, swiglu, comm_cus=comm_cus, bm=bm), m, n)
    v = (WIDE_SPLIT_VARIANT if s > 1 else WIDE_VARIANT) if variant < 0 else variant
    if bm != wide_bm(m):
        v |= bm << WIDE_ROW_TILE_SHIFT
    return GemmRoute("wide", s, v, swiglu)


def linear_wide(x: torch.Tensor, w: torch.Tensor, splits: int = 0, swiglu: bool = False, defer: bool = False,
                variant: int = -1):
    """Wide-M decode GEMM (csrc/kernels/gemm_wide.hip): 256 x 128 x 64 tiles, 3-deep LDS-DMA pipeline, optional
    split-K and fused SwiGLU epilogue (``w`` = [Wg; Wu]).  ``defer``: may return a :class:`SplitKPartial` (no SwiGLU)."""
    return _launch("gemm_wide", x, w, _wide_route(*_mnk("linear_wide", x, w, 128), swiglu, splits, variant), defer)


def pp_splits(m: int, n: int, k: int, bn: int = 256, target_wgs: int = 256) -> int:
    """K slices for gemm_pp: about one workgroup per CU (tiles x slices <= target), >= 3 K-tiles
    (192) per slice."""
    tiles = (n // bn) * (-(-m // 256))
    return max(1, min(target_wgs // max(1, tiles), (k // 64) // 3, 32))


def _pp_route(m, n, k, swiglu, splits=0, variant=0) -> GemmRoute:
    bn = 128 if variant & PP_BN128 else 256
    return GemmRoute("pp", ws_splits(splits or pp_splits(m, n, k, bn), m, n), variant, swiglu)


def linear_pp(x: torch.Tensor, w: torch.Tensor, splits: int = 0, swiglu: bool = False, defer: bool = False,
              variant: int = 0):
    """Ping-pong 256-row-tile GEMM (csrc/kernels/gemm_pp.hip); ``variant``: the PP_* bits.  Split-K partials are
    reduced by splitk_reduce(_swiglu), or returned as a :class:`SplitKPartial` with ``defer`` (no SwiGLU)."""
    bn = 128 if variant & PP_BN128 else 256
    return _launch("gemm_pp", x, w, _pp_route(*_mnk("linear_pp", x, w, bn), swiglu, splits, variant), defer)


def _pf_route(k, swiglu, variant=0, comm_cus=None) -> GemmRoute:
    return GemmRoute("pf", 0, variant | (PF_DYNAMIC if pf_dynamic(comm_cus) and k >= 128 else 0), swiglu)


def linear_pf(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False, variant: int = 0) -> torch.Tensor:
    """Persistent prefill GEMM (gemm_pf in csrc/kernels/gemm_pp.hip): schedule 2's 256 x 256 tiles, one workgroup
    per CU walking its tiles with the LDS-DMA pipeline running across tile boundaries; optional fused SwiGLU
    (``w`` = [Wg; Wu], y [M, N / 2]).  ``variant``: PF_NT_STORES; the tiles come from per-XCD device queues while
    knobs.pf_dynamic says so (PF_DYNAMIC: a stream capture clears that bit, also one the caller passed)."""
    return _launch("gemm_pf", x, w, _pf_route(_mnk("linear_pf", x, w, 256)[2], swiglu, variant))


def sq_role(n: int, k: int, swiglu: bool) -> str:
    return "gate_up" if swiglu else "down" if is_down_proj(n, k) else "head" if n > 65536 else "proj"


def use_sq(m: int, n: int, k: int, swiglu: bool = False) -> bool:
    kn = knobs.K
    roles = {t for t in kn.sq.split(",") if t and t != "none"}
    if not roles or not (kn.sq_min_m <= m <= 256) or n % 256 or k % 64:
        return False
    if not kn.sq_split and sq_splits(m, n, k) > 1:
        return False
    return "all" in roles or sq_role(n, k, swiglu) in roles


def sq_splits(m: int, n: int, k: int, target_wgs: int = 256) -> int:
    """K slices for gemm_sq: as many as keep (N / 256) x slices within one workgroup per CU, at
    least 4 K-tiles (256) per slice."""
    tiles = (n // 256) * (-(-m // 256))
    return max(1, min(target_wgs // max(1, tiles), (k // 64) // 4, 16))


def _sq_route(m, n, k, swiglu, splits=0, variant=-1) -> GemmRoute:
    return GemmRoute("sq", ws_splits(splits or sq_splits(m, n, k), m, n), SQ_VARIANT if variant < 0 else variant, swiglu)


def linear_sq(x: torch.Tensor, w: torch.Tensor, splits: int = 0, swiglu: bool = False, defer: bool = False,
              variant: int = -1):
    """256 x 256-tile decode GEMM (csrc/kernels/gemm_sq.hip); split-K partials reduced by
    splitk_reduce(_swiglu), or returned as a :class:`SplitKPartial` with ``defer`` (no SwiGLU)."""
    return _launch("gemm_sq", x, w, _sq_route(*_mnk("linear_sq", x, w, 256), swiglu, splits, variant), defer)
