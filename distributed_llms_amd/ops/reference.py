"""Plain-PyTorch implementations of every engine op.

Two roles:
  * the CPU execution path (CPU workers, the GPT-2 plumbing config, CPU tests);
  * the numerics oracle the HIP kernels are tested against (run in fp32).

They replace what the reference delegates to ``torch.matmul`` inside its
placeholder ``ModelShard.compute`` (``src/worker/node.py:24-32``) with the real
transformer-block math.

Paged-KV layout (shared with the HIP kernels, one tensor pair per layer):
  k_cache: [num_blocks, num_kv_heads, block_size, head_dim]
  v_cache: [num_blocks, num_kv_heads, head_dim, block_size]   (32-key blocks: K row / V^T element
                                                              order of csrc/kernels/common.h krow32 /
                                                              vofs, a [4][D][8] V^T tile; V stored transposed
           so the P·V MFMA reads token-contiguous 16-byte fragments)
``slot = block_id * block_size + offset`` addresses one token's K/V.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def embedding(ids: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    return weight.index_select(0, ids.long())


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (y * w.float()).to(x.dtype)


def qkv_prep(qkv: torch.Tensor, bias: Optional[torch.Tensor], q_w: Optional[torch.Tensor],
             k_w: Optional[torch.Tensor], hq: int, hkv: int, d: int, eps: float) -> torch.Tensor:
    """Qwen2 qkv bias and Qwen3 per-head q / k RMSNorm, in place on the dense qkv [T, (hq + 2 hkv) d].

    For token t and head slot s: r = f32(qkv[t, s]) + f32(bias[s]) (no bias: r = f32(qkv[t, s])), never
    rounded in between.  q slots (s < hq) with ``q_w`` and k slots (hq <= s < hq + hkv) with ``k_w``
    become dtype(r * rsqrt(mean_d(r^2) + eps) * f32(w)), one rounding as in :func:`rms_norm`; every
    other slot dtype(r).  Slots that neither the bias nor a norm touches are not written."""
    v = qkv.view(qkv.shape[0], hq + 2 * hkv, d)
    b = None if bias is None else bias.float().view(hq + 2 * hkv, d)
    for s0, s1, w in ((0, hq, q_w), (hq, hq + hkv, k_w), (hq + hkv, hq + 2 * hkv, None)):
        if b is None and w is None:
            continue
        r = v[:, s0:s1].float()
        if b is not None:
            r = r + b[s0:s1]
        if w is not None:
            r = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w.float()
        v[:, s0:s1] = r.to(qkv.dtype)
    return qkv


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor,
                       eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """residual <- x + residual ; returns (rms_norm(residual) * w, residual)."""
    r = (x.float() + residual.float())
    residual.copy_(r.to(residual.dtype))
    r = residual.float()
    y = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps)
    return (y * w.float()).to(x.dtype), residual


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w^T (+ bias); w is [out, in] (nn.Linear convention)."""
    if x.device.type == "cpu" and x.dtype in (torch.bfloat16, torch.float16):
        y = x.float() @ w.float().t()
        if bias is not None:
            y = y + bias.float()
        return y.to(x.dtype)
    return F.linear(x, w, bias)


def silu_mul(gu: torch.Tensor) -> torch.Tensor:
    """gu = [gate | up] along the last dim -> silu(gate) * up."""
    i = gu.shape[-1] // 2
    g, u = gu[..., :i].float(), gu[..., i:].float()
    return (F.silu(g) * u).to(gu.dtype)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


def rope_cos_sin(head_dim: int, max_pos: int, theta: float, scaling: Optional[dict] = None,
                 device="cpu") -> torch.Tensor:
    """[max_pos, head_dim] float32: first half cos, second half sin (rotate-half RoPE).

    Implements the ``llama3`` frequency rescaling when ``scaling['rope_type'] == 'llama3'``.
    """
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling["low_freq_factor"], scaling["high_freq_factor"]
        old = scaling["original_max_position_embeddings"]
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (wl <= lo_wl) & (wl >= hi_wl)
        scaled = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
        inv = scaled
    t = torch.arange(max_pos, dtype=torch.float64)
    freqs = torch.outer(t, inv)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).float().to(device)


def apply_rope(x: torch.Tensor, pos: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, H, D]; rotate-half convention (HF Llama)."""
    d = x.shape[-1]
    cs = cos_sin.index_select(0, pos.long())          # [T, D]
    cos, sin = cs[:, : d // 2].unsqueeze(1), cs[:, d // 2:].unsqueeze(1)
    xf = x.float()
    x1, x2 = xf[..., : d // 2], xf[..., d // 2:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(x.dtype)


def rope_q(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: Optional[torch.Tensor], num_heads: int,
           head_dim: int) -> torch.Tensor:
    """The rotated q [T, Hq, D] of a fused qkv projection."""
    t = qkv.shape[0]
    q = qkv[:, : num_heads * head_dim].view(t, num_heads, head_dim)
    return apply_rope(q, positions, cos_sin) if cos_sin is not None else q.contiguous()


def rope_cache_append(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: Optional[torch.Tensor],
                      k_cache: torch.Tensor, v_cache: torch.Tensor, slot_mapping: torch.Tensor,
                      num_heads: int, num_kv_heads: int, head_dim: int) -> torch.Tensor:
    """Split fused qkv [T, (Hq+2Hkv)D], rotate q/k, scatter k/v into the paged cache, return q."""
    t = qkv.shape[0]
    q = qkv[:, : num_heads * head_dim].view(t, num_heads, head_dim)
    k = qkv[:, num_heads * head_dim: (num_heads + num_kv_heads) * head_dim].view(t, num_kv_heads, head_dim)
    v = qkv[:, (num_heads + num_kv_heads) * head_dim:].view(t, num_kv_heads, head_dim)
    if cos_sin is not None:
        q = apply_rope(q, positions, cos_sin)
        k = apply_rope(k, positions, cos_sin)
    else:
        q = q.contiguous()
    bs = k_cache.shape[2]
    slots = slot_mapping.long()
    blk, off = slots // bs, slots % bs
    if bs == 32:
        k_cache[blk, :, _KROW32.to(off.device)[off], :] = k.to(k_cache.dtype)
        nb, hkv, d = v_cache.shape[0], v_cache.shape[1], v_cache.shape[2]
        v_cache.view(nb, hkv, 4, d, 8)[blk, :, off // 8, :, off % 8] = v.to(v_cache.dtype)
    else:
        k_cache[blk, :, off, :] = k.to(k_cache.dtype)
        v_cache[blk, :, :, off] = v.to(v_cache.dtype)
    return q


def _krow32() -> torch.Tensor:
    """Physical row of key j in a 32-key K block (csrc/kernels/common.h krow32)."""
    j = torch.arange(32)
    return ((j & 4) << 2) + ((j >> 3) << 2) + (j & 3)


_KROW32 = _krow32()


def _gather_kv(k_cache, v_cache, block_table, n):
    bs = k_cache.shape[2]
    nb = (n + bs - 1) // bs
    blocks = block_table[:nb].long()
    kb, vb = k_cache[blocks], v_cache[blocks]
    hkv, d = k_cache.shape[1], k_cache.shape[3]
    if bs == 32:
        kb = kb[:, :, _KROW32.to(kb.device), :]          # physical rows back to key order
        v = vb.reshape(nb, hkv, 4, d, 8).permute(1, 0, 2, 4, 3).reshape(hkv, nb * bs, d)[:, :n]
    else:
        v = vb.permute(1, 0, 3, 2).reshape(hkv, nb * bs, -1)[:, :n]
    k = kb.permute(1, 0, 2, 3).reshape(hkv, nb * bs, -1)[:, :n]
    return k, v  # [Hkv, n, D]


def paged_attention_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                           block_tables: torch.Tensor, seq_lens: torch.Tensor,
                           scale: float) -> torch.Tensor:
    """q [B, Hq, D] (one new token per sequence, already in the cache) -> [B, Hq, D].

    The whole batch in one gather: every sequence's first ceil(max_len / bs) blocks (table
    padding is block 0, a valid index), keys past its own length masked to -inf.
    """
    b, hq, d = q.shape
    if b == 0:
        return torch.empty_like(q)
    hkv, bs = k_cache.shape[1], k_cache.shape[2]
    lens = seq_lens[:b].long()
    n = int(lens.max())
    nb = (n + bs - 1) // bs
    blocks = block_tables[:b, :nb].long().clamp_min(0)
    kb, vb = k_cache[blocks], v_cache[blocks]               # [B, nb, Hkv, ...]
    if bs == 32:
        kb = kb[:, :, :, _KROW32.to(kb.device), :]         # physical rows back to key order
        v = vb.reshape(b, nb, hkv, 4, d, 8).permute(0, 2, 1, 3, 5, 4).reshape(b, hkv, nb * bs, d)
    else:
        v = vb.permute(0, 2, 1, 4, 3).reshape(b, hkv, nb * bs, d)
    k = kb.permute(0, 2, 1, 3, 4).reshape(b, hkv, nb * bs, d)
    qf = q.float().view(b, hkv, hq // hkv, d)
    s = torch.einsum("bhgd,bhnd->bhgn", qf, k.float()) * scale
    pad = torch.arange(nb * bs, device=q.device).view(1, 1, 1, -1) >= lens.to(q.device).view(b, 1, 1, 1)
    p = torch.softmax(s.masked_fill(pad, float("-inf")), dim=-1)
    o = torch.einsum("bhgn,bhnd->bhgd", p, v.float())
    return o.reshape(b, hq, d).to(q.dtype)


def paged_attention_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                            block_tables: torch.Tensor, cu_seqlens_q: torch.Tensor,
                            seq_lens: torch.Tensor, scale: float) -> torch.Tensor:
    """Causal varlen attention for a packed chunk of prompts.

    q [T, Hq, D]; sequence i owns q rows cu_seqlens_q[i]:cu_seqlens_q[i+1], which are its
    LAST q_len tokens out of seq_lens[i] context tokens (all already in the cache).
    """
    t, hq, d = q.shape
    hkv = k_cache.shape[1]
    out = torch.empty_like(q)
    cu = cu_seqlens_q.tolist()
    for i in range(len(cu) - 1):
        s0, s1 = cu[i], cu[i + 1]
        ql = s1 - s0
        if ql == 0:
            continue
        n = int(seq_lens[i])
        k, v = _gather_kv(k_cache, v_cache, block_tables[i], n)
        qi = q[s0:s1].float().permute(1, 0, 2).reshape(hkv, hq // hkv, ql, d)
        s = torch.einsum("hgqd,hnd->hgqn", qi, k.float()) * scale
        qpos = torch.arange(n - ql, n, device=q.device).view(ql, 1)
        kpos = torch.arange(n, device=q.device).view(1, n)
        s = s.masked_fill(kpos > qpos, float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgqn,hnd->hgqd", p, v.float())
        out[s0:s1] = o.reshape(hq, ql, d).permute(1, 0, 2).to(q.dtype)
    return out


def argmax(logits: torch.Tensor) -> torch.Tensor:
    return logits.float().argmax(dim=-1).to(torch.int32)


# ------------------------------------------------------------------ seeded sampling
# The contract of csrc/kernels/sampler.hip, in numpy with float64 masses.  Per row: int32 params
# (temp_e4, top_k, top_p_e4), a 64-bit seed and pos, the index of the token being drawn.
#   temp_e4 <= 0  the argmax (first index on ties; NaN counts as -inf; an all -inf row gives 0)
#   otherwise     x = l / T with T = temp_e4 * 1e-4, w = exp(x - x_max)
#     top-k  (0 < k < V)  keep x >= the k-th largest value; ties at the threshold are all kept
#     top-p  over the top-k survivors keep value v iff mass{x > v} <= p * Z_k (whole tie groups)
#     draw   u = (philox4x32_10((pos, 0, 0, 0), (seed_lo, seed_hi))[0] >> 8) * 2^-24; the first
#            kept index, in token order, whose inclusive cumulative kept mass exceeds u * Z_kept
#            (the last kept index if rounding leaves none).  ``uniforms`` (test hook) replaces u,
#            truncated to a multiple of 2^-24 below 1.
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Philox4x32-10.  ctr [..., 4], key [..., 2] (anything numpy turns into uint32 words; they
    broadcast against each other) -> uint32 [..., 4]."""
    import numpy as np
    c = np.asarray(ctr, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c0
        p1 = np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(_PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(_PHILOX_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sample_uniforms(seeds, pos):
    """u in [0, 1) float64 of (seed, pos) pairs; seeds: 64-bit ints (any sign), pos: ints."""
    import numpy as np
    s = np.asarray(seeds).astype(np.int64).view(np.uint64).reshape(-1)
    p = np.asarray(pos).astype(np.int64).reshape(-1)
    ctr = np.zeros((p.shape[0], 4), dtype=np.uint64)
    ctr[:, 0] = p.view(np.uint64) & np.uint64(0xFFFFFFFF)
    key = np.stack([s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)], axis=-1)
    return (philox4x32_10(ctr, key)[:, 0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def sample_rows_detail(logits, params, u, dtype=None):
    """The contract on numpy arrays: logits [B, V] floats, params [B, 3] ints, u [B] float64 ->
    (ids int32 [B], kept bool [B, V], w [B, V]).  ``kept`` / ``w`` of greedy rows and of rows
    without an entry above -inf are not meaningful.  ``dtype``: the type of the masses and their
    sums (float64; float32 is how tests measure what single precision costs)."""
    import numpy as np
    dtype = np.float64 if dtype is None else dtype
    l = np.array(logits, dtype=dtype)
    params = np.asarray(params, dtype=np.int64)
    b, v = l.shape
    l[np.isnan(l)] = -np.inf
    lmax = l.max(axis=1)
    first_max = np.argmax(l, axis=1)
    rows = np.arange(b)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (np.where(params[:, 0] > 0, params[:, 0], 1) * 1e-4).astype(dtype)
        d = l - lmax[:, None]
        d[l == lmax[:, None]] = 0.0          # inf - inf at a +inf maximum
        x = d / t[:, None]
        w = np.exp(x)
        order = np.argsort(-x, axis=1, kind="stable")
        xs = np.take_along_axis(x, order, 1)
        k = params[:, 1]
        kact = (k > 0) & (k < v)
        tau_k = xs[np.arange(b), np.clip(k, 1, v) - 1]
        keep = np.where(kact[:, None], x >= tau_k[:, None], True)
        zk = (w * keep).sum(axis=1)
        # mass strictly above each value, in sorted order: the cumulative mass before its tie group
        ws = np.take_along_axis(w * keep, order, 1)
        cum = np.cumsum(ws, axis=1)
        pos = np.broadcast_to(np.arange(v), (b, v))
        new_group = np.concatenate([np.ones((b, 1), dtype=bool), xs[:, 1:] != xs[:, :-1]], axis=1)
        start = np.maximum.accumulate(np.where(new_group, pos, 0), axis=1)
        excl = np.concatenate([np.zeros((b, 1), dtype=dtype), cum], axis=1)
        above_s = np.take_along_axis(excl, start, 1)
        p = (np.clip(params[:, 2], 0, 10000) * 1e-4).astype(dtype)
        keep_ps = np.where((params[:, 2] < 10000)[:, None], above_s <= (p * zk)[:, None], True)
        keep_p = np.empty_like(keep_ps)
        np.put_along_axis(keep_p, order, keep_ps, 1)
        kept = keep & keep_p
        mk = w * kept
        cdf = np.cumsum(mk, axis=1)
        z = cdf[:, -1]
        hit = cdf > (np.asarray(u, dtype=np.float64).astype(dtype) * z)[:, None]
        drawn = np.where(hit.any(axis=1), hit.argmax(axis=1), v - 1 - kept[:, ::-1].argmax(axis=1))
    ids = np.where((params[:, 0] <= 0) | np.isneginf(lmax), first_max, drawn)
    return ids.astype(np.int32), kept, w


def sample_rows(logits: torch.Tensor, params: torch.Tensor, seeds: torch.Tensor, pos: torch.Tensor,
                uniforms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [B, V]; params [B, 3] int32; seeds [B] int64 (the 64-bit pattern); pos [B] int32;
    uniforms [B] float32 or None -> ids [B] int32 on the logits' device."""
    import numpy as np
    lg = logits.detach().float().cpu().numpy()
    b, v = lg.shape
    pr = params.detach().cpu().numpy().reshape(b, 3)
    if uniforms is None:
        u = sample_uniforms(seeds.detach().cpu().numpy(), pos.detach().cpu().numpy())
    else:
        m = np.floor(np.clip(uniforms.detach().float().cpu().numpy().astype(np.float64), 0.0, 1.0) * 2.0 ** 24)
        u = np.minimum(m, 2.0 ** 24 - 1) * 2.0 ** -24
    ids = np.empty(b, dtype=np.int32)
    step = max(1, (1 << 22) // max(v, 1))         # bound the float64 temporaries
    for s in range(0, b, step):
        ids[s:s + step] = sample_rows_detail(lg[s:s + step], pr[s:s + step], u[s:s + step])[0]
    return torch.from_numpy(ids).to(logits.device)


# ------------------------------------------------------------------ per-token log-probabilities
# The contract of token_logprobs_kernel (csrc/kernels/sampler.hip), in numpy float64: the
# log-probabilities of the model's distribution (temperature, top-k and top-p play no part).
#   NaN counts as -inf and -0 equals +0 (the sampler's key order); m = row maximum;
#   Z = sum_j exp(x_j - m), an entry equal to m contributing exactly 1;
#   lp_i = (x_i - m) - ln Z with x_i - m = 0 where x_i == m; a row whose maximum is -inf has every
#   lp = -inf; a +inf maximum falls out: the +inf entries get -ln(count), the rest -inf.
#   want[b] < 0   the row is skipped: chosen = 0, top_ids = -1, top_lp = 0
#   want[b] = n   chosen = lp[ids[b]] (-inf, nothing read, for an id outside [0, V)); the first
#                 min(n, n_max, V) top slots hold the largest entries by decreasing value, then
#                 increasing index; the remaining slots hold -1 / 0
MAX_LOGPROBS = 20


def token_logprobs_detail(logits, ids, want, n_max: int):
    """The contract on numpy arrays: logits [B, V] floats, ids [B] and want [B] ints ->
    (chosen float64 [B], top_ids int32 [B, n_max], top_lp float64 [B, n_max])."""
    import numpy as np
    l = np.array(logits, dtype=np.float64)
    b, v = l.shape
    ids = np.asarray(ids, dtype=np.int64).reshape(b)
    want = np.asarray(want, dtype=np.int64).reshape(b)
    chosen = np.zeros(b, dtype=np.float64)
    top_ids = np.full((b, n_max), -1, dtype=np.int32)
    top_lp = np.zeros((b, n_max), dtype=np.float64)
    l[np.isnan(l)] = -np.inf
    for r in range(b):
        if want[r] < 0:
            continue
        x = l[r]
        m = x.max()
        if np.isneginf(m):
            lp = np.full(v, -np.inf)
        else:
            with np.errstate(invalid="ignore"):
                d = x - m
            d[x == m] = 0.0                      # inf - inf at a +inf maximum
            lp = d - np.log(np.exp(d).sum())
        chosen[r] = lp[ids[r]] if 0 <= ids[r] < v else -np.inf
        n = int(min(want[r], n_max, v))
        if n > 0:
            order = np.argsort(-x, kind="stable")[:n]     # -0 == +0: ties fall to the smaller index
            top_ids[r, :n] = order
            top_lp[r, :n] = lp[order]
    return chosen, top_ids, top_lp


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, want: torch.Tensor, n_max: int):
    """logits [B, V]; ids [B] int32 (the chosen tokens); want [B] int32 (-1: skip the row, else how
    many top entries) -> (chosen [B] float32, top_ids [B, n_max] int32, top_lp [B, n_max] float32)
    on the logits' device."""
    lg = logits.detach().to(torch.float64).cpu().numpy()
    c, ti, tl = token_logprobs_detail(lg, ids.detach().cpu().numpy(), want.detach().cpu().numpy(), int(n_max))
    dev = logits.device
    return (torch.from_numpy(c).to(torch.float32).to(dev), torch.from_numpy(ti).to(dev),
            torch.from_numpy(tl).to(torch.float32).to(dev))


# ------------------------------------------------------------------ logit processors
# The contract of csrc/kernels/logit_processors.hip, in numpy float32.  Two per-token quantities of
# a request drive it: in_prompt[t] (t occurs in its prompt) and n_out[t] (how often t occurs in its
# outputs so far; outputs recomputed as "prompt" after a preemption still count as outputs).  For
# every token t that some rule touches, each operation rounded to float32 on its own (no fused
# multiply-add, a correctly rounded divide):
#   x = f32(logit[t])
#   if (in_prompt[t] or n_out[t] > 0) and rep != 1:  x = x / rep if x > 0 else x * rep
#   if n_out[t] > 0:  x = x - (freq * f32(n_out[t]));  x = x - pres
#   if t in bias:     x = x + bias[t]
#   if t == eos and (index of the output token being drawn) < min_tokens:  x = -inf
#   logit[t] = round(x)   ONE rounding to the logits' type (bf16: nearest even), whatever applied
# A token no rule touches keeps its bits (-0, NaN payloads); NaN in stays NaN.  Repetition runs over
# prompt + output, presence and frequency over output only (vLLM's semantics).
#
# Device state: one int32 word per (state row, token): output count | STATE_BIAS_BIT |
# STATE_PROMPT_BIT; procs [B, PROC_WORDS] int32 per step row (PROC_* word indices below).
PROC_WORDS = 8
PROC_ROW, PROC_PROMPT_LEN, PROC_FLAGS, PROC_REP, PROC_PRES, PROC_FREQ, PROC_MIN_TOKENS, PROC_START = range(8)
PROC_SAMPLE = 1        # flag: apply the processors to the row and count the id it draws
PROC_UPDATE = 2        # flag: the row is a prefill chunk whose tokens enter the state
STATE_COUNT_MASK = 0x00FFFFFF
STATE_BIAS_BIT = 1 << 29
STATE_PROMPT_BIT = 1 << 31
MAX_LOGIT_BIAS = 300


def bf16_rne_bits(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even; NaN stays a (quiet) NaN."""
    import numpy as np
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def logit_processors_row(x, in_prompt, n_out, rep=1.0, pres=0.0, freq=0.0, bias=None, ban_id=-1):
    """The chain on one row: x [V] float32 (the logits, converted exactly), in_prompt [V] bool,
    n_out [V] ints, bias {id: value} -> (x' float32 [V], touched bool [V]); entries of x' that are
    not ``touched`` are meaningless.  ``ban_id`` >= 0: the id that min_tokens bans in this step."""
    import numpy as np
    x = np.array(x, dtype=np.float32)
    v = x.shape[0]
    n_out = np.asarray(n_out).astype(np.int64)
    rep, pres, freq = np.float32(rep), np.float32(pres), np.float32(freq)
    out = n_out > 0
    touched = out.copy()
    with np.errstate(all="ignore"):
        if rep != np.float32(1.0):
            seen = np.asarray(in_prompt, dtype=bool) | out
            touched |= seen
            x = np.where(seen, np.where(x > 0, x / rep, x * rep), x).astype(np.float32)
        f = (freq * n_out.astype(np.float32)).astype(np.float32)
        x = np.where(out, ((x - f).astype(np.float32) - pres).astype(np.float32), x)
        for t, b in (bias or {}).items():
            t = int(t)
            if 0 <= t < v:
                x[t] = x[t] + np.float32(b)
                touched[t] = True
    if 0 <= ban_id < v:
        x[ban_id] = -np.inf
        touched[ban_id] = True
    return x, touched


def _proc_f32(procs, col):
    import numpy as np
    return np.ascontiguousarray(procs[:, col]).view(np.float32)


def _state_rows(procs, flag, state_rows):
    """(step rows, their state rows) of the rows that carry ``flag`` and a valid state row."""
    import numpy as np
    sr = procs[:, PROC_ROW]
    rows = np.nonzero((sr >= 0) & (sr < state_rows) & ((procs[:, PROC_FLAGS] & flag) != 0))[0]
    return rows, sr[rows].astype(np.int64)


@torch.inference_mode()    # the engines' logits are inference tensors; in-place writes need the mode
def logit_state_update(state, vocab, ids, cu_seqlens, procs, bias_n, bias_ids, bias_vals, step_bias_cu,
                       step_bias_ids, step_bias_vals) -> None:
    """Prefill chunks enter the state (in place): a chunk that starts at position 0 zeroes its own
    state row and installs its bias list; then every chunk token at a position < prompt_len sets the
    prompt bit, every later one adds one to the count.  Ids outside [0, vocab) are ignored."""
    import numpy as np
    pr = procs.detach().cpu().numpy().reshape(-1, PROC_WORDS)
    rows, srows = _state_rows(pr, PROC_UPDATE, state.shape[0])
    if rows.shape[0] == 0:
        return
    idn, cu = ids.detach().cpu().numpy(), cu_seqlens.detach().cpu().numpy()
    bcu, bid = step_bias_cu.detach().cpu().numpy(), step_bias_ids.detach().cpu().numpy()
    for r, s in zip(rows.tolist(), srows.tolist()):
        st = state[s].detach().cpu().numpy().view(np.uint32).copy()
        start, plen = int(pr[r, PROC_START]), int(pr[r, PROC_PROMPT_LEN])
        if start == 0:
            st[:] = 0
            a, e = int(bcu[r]), int(bcu[r + 1])
            n = min(e - a, bias_ids.shape[1])
            bias_n[s] = n
            bias_ids[s, :n] = step_bias_ids[a:a + n]
            bias_vals[s, :n] = step_bias_vals[a:a + n]
            b = bid[a:a + n]
            st[b[(b >= 0) & (b < vocab)]] |= np.uint32(STATE_BIAS_BIT)
        toks = idn[int(cu[r]):int(cu[r + 1])].astype(np.int64)
        pos = start + np.arange(toks.shape[0])
        ok = (toks >= 0) & (toks < vocab)
        st[toks[ok & (pos < plen)]] |= np.uint32(STATE_PROMPT_BIT)
        np.add.at(st, toks[ok & (pos >= plen)], np.uint32(1))
        state[s] = torch.from_numpy(st.view(np.int32)).to(state.device)


@torch.inference_mode()    # the engines' logits are inference tensors; in-place writes need the mode
def apply_logit_processors(logits, state, procs, seq_lens, eos_id, bias_n, bias_ids, bias_vals) -> None:
    """The chain above on every row with PROC_SAMPLE and a state row, in place (logits [B, V] of any
    float type: bf16 rows are rounded to nearest even, float32 rows not at all)."""
    import numpy as np
    pr = procs.detach().cpu().numpy().reshape(-1, PROC_WORDS)
    rows, srows = _state_rows(pr, PROC_SAMPLE, state.shape[0])
    if rows.shape[0] == 0:
        return
    v = logits.shape[1]
    sl = seq_lens.detach().cpu().numpy()
    rep, pres, freq = _proc_f32(pr, PROC_REP), _proc_f32(pr, PROC_PRES), _proc_f32(pr, PROC_FREQ)
    bn, bi, bv = (t.detach().cpu().numpy() for t in (bias_n, bias_ids, bias_vals))
    for r, s in zip(rows.tolist(), srows.tolist()):
        st = state[s, :v].detach().cpu().numpy().view(np.uint32)
        n = int(bn[s])
        bias = {int(t): np.float32(b) for t, b in zip(bi[s, :n], bv[s, :n])}
        ban = int(eos_id) if eos_id >= 0 and int(sl[r]) - int(pr[r, PROC_PROMPT_LEN]) < int(pr[r, PROC_MIN_TOKENS]) else -1
        row = logits[r]
        x, touched = logit_processors_row(row.detach().float().cpu().numpy(), (st & np.uint32(STATE_PROMPT_BIT)) != 0,
                                          st & np.uint32(STATE_COUNT_MASK), rep[r], pres[r], freq[r], bias, ban)
        if not touched.any():
            continue
        if row.dtype == torch.bfloat16:
            old = row.detach().view(torch.int16).cpu().numpy().view(np.uint16)
            new = np.where(touched, bf16_rne_bits(x), old)
            row.copy_(torch.from_numpy(new.view(np.int16)).view(torch.bfloat16).to(row.device))
        else:
            idx = torch.from_numpy(np.nonzero(touched)[0]).to(row.device)
            row[idx] = torch.from_numpy(x[touched]).to(row.device, row.dtype)


@torch.inference_mode()    # the engines' logits are inference tensors; in-place writes need the mode
def logit_state_count(state, vocab, ids, procs) -> None:
    """After sampling: every row with PROC_SAMPLE and a state row counts the id it drew (in place)."""
    pr = procs.detach().cpu().numpy().reshape(-1, PROC_WORDS)
    rows, srows = _state_rows(pr, PROC_SAMPLE, state.shape[0])
    idn = ids.detach().cpu().numpy()
    for r, s in zip(rows.tolist(), srows.tolist()):
        t = int(idn[r])
        if 0 <= t < vocab:
            state[s, t] += 1


def moe_route(router_logits: torch.Tensor, top_k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mixtral routing: softmax over experts, top-k, renormalise. -> (weights f32, ids i32)."""
    probs = torch.softmax(router_logits.float(), dim=-1)
    w, ids = torch.topk(probs, top_k, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    return w, ids.to(torch.int32)


def moe_mlp(x: torch.Tensor, w_gate_up: torch.Tensor, w_down: torch.Tensor,
            topk_w: torch.Tensor, topk_ids: torch.Tensor) -> torch.Tensor:
    """x [T,H]; w_gate_up [E, 2I, H]; w_down [E, H, I] -> [T, H] (weighted sum over top-k)."""
    t, h = x.shape
    out = torch.zeros(t, h, dtype=torch.float32, device=x.device)
    for e in range(w_gate_up.shape[0]):
        tok, slot = (topk_ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        gu = linear(x[tok], w_gate_up[e])
        y = linear(silu_mul(gu), w_down[e])
        out.index_add_(0, tok, y.float() * topk_w[tok, slot].unsqueeze(1).float())
    return out.to(x.dtype)


# ------------------------------------------------------------ multi-LoRA
# Per-row adapters as an additive delta after a projection (the HIP kernels of csrc/kernels/lora.hip
# compute the same thing; the CPU engine runs this).  The projection's base output is y0 = dtype(x W^T)
# as the GEMM leaves it once materialised.  Row t carries adapter slot a = slot[t]; a row with
# a = -1 is untouched.  For the others
#     v[t, j] = dtype( sum_k x[t, k] A_a[j, k] )            f32 accumulation, one rounding
#     d[t, n] = sum_j v[t, j] B_a[n, j]                      f32
#     y[t, n] = dtype( f32(y0[t, n]) + scale_a d[t, n] )     one rounding
# scale_a = lora_alpha / r (lora_alpha / sqrt(r) with use_rslora) stays an f32 per slot, applied in the
# epilogue, never folded into B.  A packed projection (q|k|v with unequal widths under GQA, gate|up)
# holds one LoRA module per slice over the same input: A is stacked to [slots, nslices * rp, K] (rp:
# the rank zero-padded, LORA_RANK_PAD), B is [slots, N, rp] with row n from the module that owns
# output column n, and column n takes the v slice of that module.  A module the adapter does not
# target is a zero slice.
LORA_TILE = 16            # rows of a row-plan tile
LORA_MAX_RANK = 64


def lora_rank_pad(rank: int) -> int:
    """The stored rank: zero-padded to what the MFMA shapes take (32 or 64)."""
    if not 1 <= rank <= LORA_MAX_RANK:
        raise ValueError(f"LoRA rank must be in [1, {LORA_MAX_RANK}], got {rank}")
    return 32 if rank <= 32 else 64


def lora_scale(lora_alpha: float, rank: int, use_rslora: bool = False) -> float:
    return float(lora_alpha) / (math.sqrt(rank) if use_rslora else rank)


def lora_apply(y0: torch.Tensor, x: torch.Tensor, slot: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
               scale: torch.Tensor, slice_starts=(0,)) -> torch.Tensor:
    """y0 [T, N] and x [T, K] in the engine's dtype, slot [T] int, a [slots, nslices * rp, K], b
    [slots, N, rp], scale [slots] float32, slice_starts: first output column of every slice.  Returns
    a new tensor; rows with slot -1 are copied bit for bit."""
    t, n = y0.shape
    rp = b.shape[-1]
    starts = list(slice_starts) + [n]
    if a.shape[1] != rp * (len(starts) - 1):
        raise ValueError("lora_apply: A must stack one rp-row block per slice")
    y = y0.clone()
    slot = slot.to(torch.int64)
    for s in sorted(set(slot.tolist())):
        if s < 0:
            continue
        rows = (slot == s).nonzero().flatten()
        xs = x.index_select(0, rows)
        v = (xs.float() @ a[s].float().t()).to(x.dtype).float()          # [n_rows, nslices * rp]
        d = torch.empty(rows.numel(), n, dtype=torch.float32, device=y0.device)
        for i in range(len(starts) - 1):
            c0, c1 = starts[i], starts[i + 1]
            d[:, c0:c1] = v[:, i * rp:(i + 1) * rp] @ b[s, c0:c1].float().t()
        y[rows] = (y0.index_select(0, rows).float() + scale[s].float() * d).to(y0.dtype)
    return y
