"""Paged attention on the host (csrc/kernels/attention.hip): RoPE + cache append, the split planners, the
prefill route -- decided once, by :func:`prefill_route`; the native launcher runs the version it is given --
and the decode / prefill wrappers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .. import _ext, knobs
from . import _ck, _gpu, _stream, gemm
from . import reference as ref


# ----------------------------------------------------------- K4 + K5
def _ck_rope(width: int, cos_sin, num_heads: int, num_kv_heads: int, head_dim: int):
    if width != (num_heads + 2 * num_kv_heads) * head_dim:
        raise ValueError("qkv width mismatch")
    if cos_sin is not None:
        _ck(cos_sin, "cos_sin", torch.float32)
        if cos_sin.shape[1] != head_dim:
            raise ValueError("cos_sin width must equal head_dim")


def rope_cache_append(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, num_heads, num_kv_heads,
                      head_dim, write_q: bool = True) -> Optional[torch.Tensor]:
    """Rotate k (and q) and append k / v^T to the paged cache; returns the rotated q [T, Hq, D], or
    None with ``write_q=False`` (the prefill attention then rotates q itself)."""
    if not _gpu(qkv):
        q = ref.rope_cache_append(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, num_heads,
                                  num_kv_heads, head_dim)
        return q if write_q else None
    _ck(qkv, "rope.qkv")
    _ck(k_cache, "k_cache")
    _ck(v_cache, "v_cache")
    _ck(positions, "positions", torch.int32)
    _ck(slot_mapping, "slot_mapping", torch.int32)
    t = qkv.shape[0]
    _ck_rope(qkv.shape[1], cos_sin, num_heads, num_kv_heads, head_dim)
    q = torch.empty(t, num_heads, head_dim, dtype=qkv.dtype, device=qkv.device) if write_q else None
    _ext.kernels().rope_cache_append(q.data_ptr() if write_q else 0, qkv.data_ptr(), positions.data_ptr(),
                                     0 if cos_sin is None else cos_sin.data_ptr(), k_cache.data_ptr(),
                                     v_cache.data_ptr(), slot_mapping.data_ptr(), t, num_heads, num_kv_heads,
                                     head_dim, k_cache.shape[2], int(knobs.K.v_group_append), _stream())
    return q


# ---------------------------------------------------------- K6 / K7
MAX_DECODE_SPLITS = 64       # splits of a sequence's keys at the most: bounds the partial workspace


def decode_split_plan(batch: int, num_kv_heads: int, max_ctx: int, block_size: int = 32,
                      max_blocks: Optional[int] = None, target_waves: Optional[int] = None) -> Tuple[int, int]:
    """(num_splits, split_len) for the decode kernel (one wave per split x kv-head x sequence).

    Aim for ~8 waves per CU (256 CUs) with >= 2 KV blocks per split so each wave's load
    pipeline has something to overlap.  The split BOUNDARIES depend only on the pow2-bucketed
    batch x kv-heads and on the block-table width -- not on ``max_ctx`` -- so a graph replayed
    at a padded (batch, context) bucket and the eager path partition every sequence's keys
    identically: the extra splits of the bucket are empty and add exact zeros, and the two
    paths produce bit-identical attention.
    """
    target_waves = target_waves or knobs.K.attn_target_waves     # sweep: profiles/attn_decode_sweep.txt
    max_blocks = max_blocks or -(-max_ctx // block_size)
    pairs = 1 << max(0, (max(1, batch * num_kv_heads) - 1).bit_length())
    target = max(1, min(MAX_DECODE_SPLITS, target_waves // pairs))
    split_len = block_size * max(2, -(-max_blocks // target))
    splits = max(1, -(-max_ctx // split_len))
    return splits, split_len


def _into(out: Optional[torch.Tensor], y: torch.Tensor) -> torch.Tensor:
    if out is None:
        return y
    out.copy_(y)
    return out


def _out_like(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.shape != shape or not out.is_contiguous() or out.dtype != dtype:
        raise ValueError("attention out must be a contiguous tensor shaped like q")
    return out


def _partials(workspace: Optional[tuple], rows: int, num_heads: int, head_dim: int, splits: int, device):
    """Pointers of the split kernels' (o, ml) partial buffers, [rows, Hq, splits, D] and [rows, Hq,
    splits, 2] floats: ``workspace`` checked for size, or allocated for the call."""
    n = rows * num_heads * splits
    po, pml = workspace or decode_workspace(rows, num_heads, head_dim, device, splits)
    if po.numel() < n * head_dim or pml.numel() < n * 2:
        raise ValueError("attention workspace too small")
    return po.data_ptr(), pml.data_ptr()


def decode_workspace(max_batch: int, num_heads: int, head_dim: int, device, splits: int = MAX_DECODE_SPLITS):
    """An (o, ml) workspace; with the default ``splits`` it serves every decode call of up to ``max_batch``
    sequences (a captured graph keeps one: the plan never exceeds MAX_DECODE_SPLITS)."""
    n = max_batch * num_heads * splits
    return (torch.empty(n * head_dim, dtype=torch.float32, device=device),
            torch.empty(n * 2, dtype=torch.float32, device=device))


def _decode(b, q, rope, k_cache, v_cache, block_tables, seq_lens, num_heads, head_dim, scale, max_ctx, workspace, out,
            dtype, device):
    """Both decode wrappers.  ``rope``: None (``q`` is the rotated [B, Hq, D]) or (qkv, part, positions,
    cos_sin, slot_mapping) for the kernel with RoPE + append fused in."""
    _ck(k_cache, "k_cache")
    _ck(v_cache, "v_cache")
    _ck(block_tables, "block_tables", torch.int32)
    _ck(seq_lens, "seq_lens", torch.int32)
    hq, d, hkv, bs = num_heads, head_dim, k_cache.shape[1], k_cache.shape[2]
    max_blocks = block_tables.shape[1]
    if max_ctx is None:
        max_ctx = max_blocks * bs
    if max_ctx > max_blocks * bs:
        raise ValueError("max_ctx exceeds block table capacity")
    splits, split_len = decode_split_plan(b, hkv, max_ctx, bs, max_blocks)
    out = _out_like(out, (b, hq, d), dtype, device)
    po, pml = _partials(workspace, b, hq, d, splits, device) if splits > 1 else (0, 0)
    tail = (block_tables.data_ptr(), seq_lens.data_ptr(), po, pml, b, hq, hkv, d, bs, max_blocks, splits, split_len,
            float(scale))
    if rope is None:
        _ext.kernels().paged_attention_decode(out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                              *tail, _stream())
        return out
    qkv, part, positions, cos_sin, slot_mapping = rope
    _ext.kernels().paged_attention_decode_rope(
        out.data_ptr(), 0 if part is not None else qkv.data_ptr(), positions.data_ptr(),
        0 if cos_sin is None else cos_sin.data_ptr(), slot_mapping.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        *tail, 0 if part is None else part.ws.data_ptr(), 0 if part is None else part.splits,
        0 if part is None else part.m * part.n, _stream())
    return out


def paged_attention_decode(q, k_cache, v_cache, block_tables, seq_lens, scale: float,
                           max_ctx: Optional[int] = None, workspace: Optional[tuple] = None,
                           out: Optional[torch.Tensor] = None):
    """``out``: write the result there (a contiguous [B, Hq, D] view, e.g. rows of a mixed step)."""
    if not _gpu(q):
        return _into(out, ref.paged_attention_decode(q, k_cache, v_cache, block_tables, seq_lens, scale))
    _ck(q, "attn.q")
    return _decode(q.shape[0], q, None, k_cache, v_cache, block_tables, seq_lens, q.shape[1], q.shape[2], scale, max_ctx,
                   workspace, out, q.dtype, q.device)


def paged_attention_decode_rope(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, block_tables, seq_lens,
                                num_heads: int, num_kv_heads: int, head_dim: int, scale: float,
                                max_ctx: Optional[int] = None, workspace: Optional[tuple] = None):
    """Decode attention with RoPE + KV-cache append fused in (one launch instead of two): reads the raw
    qkv projection [B, (Hq + 2 Hkv) * D], appends each sequence's new k / v at ``slot_mapping`` and
    attends over the whole context including it.  Same result as ``rope_cache_append`` followed by
    ``paged_attention_decode`` (the new key is folded in last instead of inside its block).

    ``qkv`` may be a :class:`gemm.SplitKPartial`: the kernel then sums the split-K slabs (f32 sums of f16 x 2^-6 slices) itself
    (bit-identical to reducing first), which removes the reduce launch and the bf16 round trip."""
    part = qkv if isinstance(qkv, gemm.SplitKPartial) else None
    if part is not None and len(part.shape) != 2:
        raise ValueError("qkv partial must be [B, (Hq + 2 Hkv) * D]")
    b, width = (part.m, part.n) if part is not None else (qkv.shape[0], qkv.shape[-1])
    if part is None and not _gpu(qkv):
        q = ref.rope_cache_append(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, num_heads, num_kv_heads,
                                  head_dim)
        return ref.paged_attention_decode(q, k_cache, v_cache, block_tables, seq_lens, scale)
    if part is None:
        _ck(qkv, "attn.qkv")
    _ck(positions, "positions", torch.int32)
    _ck(slot_mapping, "slot_mapping", torch.int32)
    _ck_rope(width, cos_sin, num_heads, num_kv_heads, head_dim)
    return _decode(b, None, (qkv, part, positions, cos_sin, slot_mapping), k_cache, v_cache, block_tables, seq_lens,
                   num_heads, head_dim, scale, max_ctx, workspace, None, qkv.dtype, qkv.device)


# ------------------------------------------------------------ prefill: the rules
PREFILL_SPLIT = 5            # the split-context prefill kernel's version number
PF_SPLIT_MIN_CHUNKS = 8      # KV chunks (of 32 keys) a split walks at least: its load pipeline needs a run
PF_SPLIT_TARGET_WGS = 512    # workgroups to aim for: two per CU
PF_SPLIT_MAX_PLAIN_WGS = 128  # the plain grid "cannot fill the device": at most half the CUs
PF_SPLIT_MAX_Q = 64          # query rows per sequence up to which the cutover was measured (profiles/prefix_cache.md)
KV_BLOCK = 32              # attention.hip kBS: tokens per KV block, the only size the kernels take
PF_MAX_CHUNKS = 1024    # attention.hip kPfMaxChunks: the LDS prefill kernels stage <= 32k tokens of block ids
PF_LDS_VERSIONS = (4, 7, 9)  # the LDS kernels: they take the raw qkv projection and rotate q themselves


def prefill_attn_version(max_q_len: int, head_dim: int) -> int:
    """The prefill attention kernel for a batch: knobs.prefill_attn, or with 0 (auto) from
    knobs.prefill_w32_min_q query rows at head_dim 128 the persistent 32x32x16 kernel (9: 1.1x v4 at
    64 x 512-token prompts, 1.35x at 1 x 16k; profiles/round6_attention.md) -- or its one-shot form (7)
    while spinning comm kernels hold CUs (ops.gemm.reserve_cus_for_comm: a persistent grid sized to
    every CU would wait for them) -- and v4 below (256 x 128-token prompts: v4 180-185 us, v9 185-193)."""
    v = knobs.K.prefill_attn
    if v:
        return v
    if head_dim != 128 or max_q_len < knobs.K.prefill_w32_min_q:
        return 4
    return 7 if gemm.comm_cus() else 9


def _prefill_plain_wgs(batch: int, num_kv_heads: int, max_q_len: int, group: int) -> int:
    """Workgroups of the 16x16 prefill kernels' grid (launch_prefill: 4 waves x 2 tiles x 16/G rows)."""
    rows_per_wg = 4 * max(1, 16 // group) * 2
    return -(-max_q_len // rows_per_wg) * num_kv_heads * batch


def prefill_split_plan(batch: int, num_kv_heads: int, max_q_len: int, max_ctx: int, group: int,
                       block_size: int = 32) -> Tuple[int, int]:
    """(nsplit, split_chunks) of the split-context prefill kernel, chosen as decode_split_plan chooses:
    enough splits to fill the CUs (PF_SPLIT_TARGET_WGS workgroups over the kernel's own grid, which puts
    one tile on a wave while the rows fit one workgroup), with a floor of PF_SPLIT_MIN_CHUNKS chunks per
    split.  Split s covers the chunks [s, s + 1) x split_chunks of every sequence."""
    rows1 = 4 * max(1, 16 // group)
    rows_per_wg = rows1 if max_q_len <= rows1 else 2 * rows1
    wgs = max(1, -(-max_q_len // rows_per_wg) * num_kv_heads * batch)
    chunks = max(1, -(-max_ctx // block_size))
    nsplit = max(1, min(-(-PF_SPLIT_TARGET_WGS // wgs), chunks // PF_SPLIT_MIN_CHUNKS))
    split_chunks = -(-chunks // nsplit)
    return -(-chunks // split_chunks), split_chunks


def prefill_split_eligible(batch: int, num_kv_heads: int, max_q_len: int, max_ctx: Optional[int], group: int) -> bool:
    """Whether a prefill call takes the split-context kernel by default: a short tail (at most
    PF_SPLIT_MAX_Q query rows per sequence -- the range the cutover was measured in; longer chunks of a
    chunked prompt keep the kernel they had), a plain grid that cannot fill the device (few sequences: at
    most PF_SPLIT_MAX_PLAIN_WGS workgroups), a longest context that reaches knobs.prefill_split_min_ctx
    (0: never) and a plan with more than one split.  The rule also bounds the partial workspace:
    T <= 32 x PF_SPLIT_MAX_PLAIN_WGS rows."""
    min_ctx = knobs.K.prefill_split_min_ctx
    if not min_ctx or not max_ctx or max_ctx < min_ctx or knobs.K.prefill_attn != 0:
        return False
    if max_q_len > PF_SPLIT_MAX_Q:
        return False
    if group not in (1, 2, 4, 8, 16) or _prefill_plain_wgs(batch, num_kv_heads, max_q_len, group) > PF_SPLIT_MAX_PLAIN_WGS:
        return False
    return prefill_split_plan(batch, num_kv_heads, max_q_len, max_ctx, group)[0] > 1


# ------------------------------------------------------------ prefill: the route
@dataclass(frozen=True)
class PrefillRoute:
    """What one prefill attention call runs.  ``version``: the kernel (3, 4, 5, 7 or 9);
    ``rope_in_kernel``: the kernel reads the raw qkv projection and rotates q itself (the caller appends
    with ``write_q=False`` and calls paged_attention_prefill_rope), else it reads a rotated q; ``nsplit``,
    ``split_chunks``: the plan of version 5 (0, 0 while the longest context is unknown), 1, 0 otherwise."""
    version: int
    rope_in_kernel: bool
    nsplit: int = 1
    split_chunks: int = 0


def prefill_route(batch: int, num_heads: int, num_kv_heads: int, head_dim: int, max_q_len: int,
                  max_ctx: Optional[int], max_blocks: int, *, version: int = 0, nsplit: Optional[int] = None,
                  allow_rope_in_kernel: bool = True) -> PrefillRoute:
    """The route of a prefill call over ``batch`` sequences of at most ``max_q_len`` new rows and ``max_ctx``
    keys (None: unknown to the host) behind block tables ``max_blocks`` wide.  Pure: shapes and knobs in.
    ``version`` forces a kernel; otherwise knobs.prefill_attn == 5 forces the split-context kernel, a call
    that is prefill_split_eligible takes it, and every other call takes prefill_attn_version.  The 32x32
    kernels (7, 9) exist for head_dim 128 and groups up to 16 (else 4), and the LDS kernels stage at most
    PF_MAX_CHUNKS block ids per sequence (else 3, the register-tiled kernel, which reads a rotated q).
    ``nsplit`` forces version 5's split count (tests, benchmarks; also more splits than chunks, the trailing
    ones empty).  ``allow_rope_in_kernel=False``: the caller has a rotated q anyway (a mixed step)."""
    group = num_heads // num_kv_heads
    version = version or (PREFILL_SPLIT if knobs.K.prefill_attn == PREFILL_SPLIT else 0)
    if version == PREFILL_SPLIT or (not version and
                                    prefill_split_eligible(batch, num_kv_heads, max_q_len, max_ctx, group)):
        if max_ctx is None:
            return PrefillRoute(PREFILL_SPLIT, False, 0, 0)
        if nsplit is None:
            return PrefillRoute(PREFILL_SPLIT, False, *prefill_split_plan(batch, num_kv_heads, max_q_len, max_ctx,
                                                                          group))
        if int(nsplit) < 1:
            raise ValueError("nsplit >= 1")
        return PrefillRoute(PREFILL_SPLIT, False, int(nsplit), max(1, -(-max(1, -(-max_ctx // KV_BLOCK)) // int(nsplit))))
    version = version or prefill_attn_version(max_q_len, head_dim)
    if version in (7, 9) and (head_dim != 128 or group > 16):
        version = 4
    if version in PF_LDS_VERSIONS and max_blocks > PF_MAX_CHUNKS:
        version = 3
    return PrefillRoute(version, bool(allow_rope_in_kernel and knobs.K.prefill_fused_rope
                                      and knobs.K.prefill_attn in (0,) + PF_LDS_VERSIONS
                                      and version in PF_LDS_VERSIONS))


# ------------------------------------------------------------ prefill: the wrappers
def _prefill_split(out, q, tensors, b, hkv, bs, max_blocks, max_q_len, max_ctx, scale, route, nsplit, workspace):
    """Version 5.  ``route`` carries the plan, unless the host does not know the longest context."""
    t, hq, d = q.shape
    if max_ctx is None:         # read it, then plan
        max_ctx = int(tensors[-1].max().item())
        route = prefill_route(b, hq, hkv, d, max_q_len, max_ctx, max_blocks, version=PREFILL_SPLIT, nsplit=nsplit)
    if max_ctx > max_blocks * bs:
        raise ValueError("max_ctx exceeds block table capacity")
    po, pml = _partials(workspace, t, hq, d, route.nsplit, q.device)
    _ext.kernels().paged_attention_prefill_split(out.data_ptr(), q.data_ptr(), *(x.data_ptr() for x in tensors), po, pml,
                                                 b, t, hq, hkv, d, bs, max_blocks, max_q_len, int(max_ctx),
                                                 route.nsplit, route.split_chunks, float(scale), _stream())
    return out


def _prefill(src, rope, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens, num_heads, head_dim, scale,
             max_q_len, out, route, version=0, max_ctx=None, nsplit=None, workspace=None):
    """Both prefill wrappers.  ``rope``: None (``src`` is the rotated q [T, Hq, D]) or (positions, cos_sin)
    with ``src`` the raw qkv projection [T, (Hq + 2 Hkv) * D]."""
    _ck(k_cache, "k_cache")
    _ck(v_cache, "v_cache")
    _ck(block_tables, "block_tables", torch.int32)
    _ck(cu_seqlens_q, "cu_seqlens_q", torch.int32)
    _ck(seq_lens, "seq_lens", torch.int32)
    tensors = (k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens)
    t, b, hq, d = src.shape[0], seq_lens.shape[0], num_heads, head_dim
    hkv, bs, max_blocks = k_cache.shape[1], k_cache.shape[2], block_tables.shape[1]
    if max_q_len is None:
        max_q_len = (cu_seqlens_q[1:] - cu_seqlens_q[:-1]).max().item() if b else 0
    max_q_len = int(max_q_len)
    if route is None:
        route = prefill_route(b, hq, hkv, d, max_q_len, max_ctx, max_blocks, version=version, nsplit=nsplit,
                              allow_rope_in_kernel=rope is not None)
    if route.rope_in_kernel != (rope is not None):
        raise ValueError("in-kernel prefill RoPE needs an LDS prefill kernel (knobs.prefill_attn 0, 4, 7 or 9) and "
                         f"block tables of <= {PF_MAX_CHUNKS} blocks; the other kernels read a rotated q")
    out = _out_like(out, (t, hq, d), src.dtype, src.device)
    if route.version == PREFILL_SPLIT:
        if t == 0 or b == 0:
            return out
        return _prefill_split(out, src, tensors, b, hkv, bs, max_blocks, max_q_len, max_ctx, scale, route, nsplit,
                              workspace)
    positions, cos_sin = rope or (None, None)
    _ext.kernels().paged_attention_prefill(out.data_ptr(), src.data_ptr(), *(x.data_ptr() for x in tensors), b, hq, hkv,
                                           d, bs, max_blocks, max_q_len, float(scale), route.version,
                                           0 if positions is None else positions.data_ptr(),
                                           0 if cos_sin is None else cos_sin.data_ptr(),
                                           src.shape[1] if rope else 0, _stream())
    return out


def paged_attention_prefill(q, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens, scale: float,
                            max_q_len: Optional[int] = None, version: int = 0, out: Optional[torch.Tensor] = None,
                            max_ctx: Optional[int] = None, nsplit: Optional[int] = None,
                            workspace: Optional[tuple] = None, route: Optional[PrefillRoute] = None):
    """Prefill attention over a rotated q [T, Hq, D].  ``route``: the call's prefill_route where the caller
    has it; otherwise built here from ``version`` (prefill kernel 3, 4, 5, 7 or 9; 0: the default),
    ``nsplit`` and ``max_ctx`` -- the batch's longest context, known to the host.  ``out`` as
    paged_attention_decode.  Version 5 is the split-context kernel (every row of q must belong to a
    sequence): ``workspace`` its (o, ml) partial buffers (None: allocated for the call)."""
    if not _gpu(q):
        return _into(out, ref.paged_attention_prefill(q, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens,
                                                      scale))
    _ck(q, "attn.q")
    return _prefill(q, None, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens, q.shape[1], q.shape[2], scale,
                    max_q_len, out, route, version, max_ctx, nsplit, workspace)


def paged_attention_prefill_rope(qkv, positions, cos_sin, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens,
                                 num_heads: int, head_dim: int, scale: float, max_q_len: Optional[int] = None,
                                 out: Optional[torch.Tensor] = None, route: Optional[PrefillRoute] = None):
    """Prefill attention reading q straight from the qkv projection [T, (Hq + 2 Hkv) * D] and rotating it
    in registers (K / V already appended by ``rope_cache_append(..., write_q=False)``): the rotated q
    never round-trips through HBM.  Returns [T, Hq, D].  ``route`` as paged_attention_prefill; it must
    say ``rope_in_kernel``."""
    if not _gpu(qkv):
        q = ref.rope_q(qkv, positions, cos_sin, num_heads, head_dim)
        return _into(out, ref.paged_attention_prefill(q, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens,
                                                      scale))
    _ck(qkv, "attn.qkv")
    _ck(positions, "positions", torch.int32)
    _ck_rope(qkv.shape[1], cos_sin, num_heads, k_cache.shape[1], head_dim)
    return _prefill(qkv, (positions, cos_sin), k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens, num_heads,
                    head_dim, scale, max_q_len, out, route)
