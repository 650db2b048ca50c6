"""Engine ops: HIP/CDNA4 kernels for GPU tensors, PyTorch reference for CPU tensors.

Device dispatch only (no backend choice on the GPU): a CUDA tensor always goes to the
in-tree ``_C_kernels`` module and raises if it is not built -- there is no silent
eager fallback on the GPU.  Every GEMM of the forward path is hand-written too (ops/gemm.py:
gemm_wide / gemm_sq for decode-sized M, the persistent gemm_pf for prefill-sized M); torch's
F.linear remains only for shapes none of them takes (a bias, N not a multiple of 256).

Every wrapper checks dtype/contiguity/shape on the host before launching, and launches
on torch's current stream so the whole decode step can be captured in a HIP graph.
"""
from __future__ import annotations

from typing import Optional, Tuple


import torch

from .. import _ext, knobs
from . import gemm, lora, quant
from . import reference as ref

__all__ = [
    "embedding", "rms_norm", "fused_add_rms_norm", "layer_norm", "linear", "silu_mul",
    "gelu_tanh", "rope_cache_append", "paged_attention_decode", "paged_attention_prefill",
    "argmax", "add_", "moe_route", "moe_mlp", "decode_split_plan", "paged_attention_decode_rope",
    "paged_attention_prefill_rope", "sample_rows", "token_logprobs", "logit_state_update",
    "apply_logit_processors", "logit_state_count", "prefill_split_plan", "prefill_split_eligible", "qkv_prep_",
]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ck(t: torch.Tensor, name: str, dtype=torch.bfloat16):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# --------------------------------------------------------------------- K1
def embedding(ids: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    if not _gpu(weight):
        return ref.embedding(ids, weight)
    _ck(weight, "embedding.weight")
    _ck(ids, "embedding.ids", torch.int32)
    t, (v, h) = ids.numel(), weight.shape
    out = torch.empty(t, h, dtype=weight.dtype, device=weight.device)
    _ext.kernels().embedding(out.data_ptr(), ids.data_ptr(), weight.data_ptr(), t, h, v, _stream())
    return out


# --------------------------------------------------------------------- K2
def _q8_out(x_like: torch.Tensor):
    h = x_like.shape[-1]
    m = x_like.numel() // h
    return (torch.empty(m, h, dtype=quant.FP8, device=x_like.device),
            torch.empty(m, dtype=torch.float32, device=x_like.device))


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, quant_out: bool = False):
    """``quant_out``: return the output as a per-token e4m3 :class:`quant.Fp8Act` for a W8A8 GEMM
    (quantized in the norm kernel's epilogue on the GPU)."""
    if not _gpu(x):
        y = ref.rms_norm(x, w, eps)
        return quant.Fp8Act(*quant.quantize_rows_ref(y), y.shape, y.dtype) if quant_out else y
    _ck(x, "rms_norm.x")
    _ck(w, "rms_norm.w")
    h = x.shape[-1]
    if quant_out:
        q, s = _q8_out(x)
        _ext.kernels().rms_norm_q8(0, x.data_ptr(), 0, w.data_ptr(), x.numel() // h, h, float(eps), q.data_ptr(),
                                   s.data_ptr(), _stream())
        return quant.Fp8Act(q, s, x.shape, x.dtype)
    y = torch.empty_like(x)
    _ext.kernels().rms_norm(y.data_ptr(), x.data_ptr(), 0, w.data_ptr(), x.numel() // h, h, float(eps), _stream())
    return y


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor,
                       eps: float, quant_out: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """residual <- x + residual (in place); returns (rms_norm(residual) * w, residual).

    ``x`` may be a :class:`gemm.SplitKPartial` (split-K GEMM output not yet reduced): the
    reduction then happens inside the same kernel (splitk_add_rms_norm).  ``quant_out``: the
    normalised output comes back as a :class:`quant.Fp8Act` (see :func:`rms_norm`)."""
    if isinstance(x, gemm.SplitKPartial):
        _ck(residual, "fused_add_rms_norm.residual")
        _ck(w, "fused_add_rms_norm.w")
        if tuple(x.shape) != tuple(residual.shape):
            raise ValueError("x/residual shape mismatch")
        if quant_out:
            q, s = _q8_out(residual)
            _ext.kernels().splitk_add_rms_norm_q8(0, residual.data_ptr(), x.ws.data_ptr(), x.splits, x.m, x.n,
                                                  w.data_ptr(), float(eps), q.data_ptr(), s.data_ptr(), _stream())
            return quant.Fp8Act(q, s, residual.shape, residual.dtype), residual
        y = torch.empty_like(residual)
        _ext.kernels().splitk_add_rms_norm(y.data_ptr(), residual.data_ptr(), x.ws.data_ptr(), x.splits, x.m, x.n,
                                           w.data_ptr(), float(eps), _stream())
        return y, residual
    if not _gpu(x):
        y, residual = ref.fused_add_rms_norm(x, residual, w, eps)
        return (quant.Fp8Act(*quant.quantize_rows_ref(y), y.shape, y.dtype) if quant_out else y), residual
    _ck(x, "fused_add_rms_norm.x")
    _ck(residual, "fused_add_rms_norm.residual")
    _ck(w, "fused_add_rms_norm.w")
    if x.shape != residual.shape:
        raise ValueError("x/residual shape mismatch")
    h = x.shape[-1]
    if quant_out:
        q, s = _q8_out(x)
        _ext.kernels().rms_norm_q8(0, x.data_ptr(), residual.data_ptr(), w.data_ptr(), x.numel() // h, h,
                                   float(eps), q.data_ptr(), s.data_ptr(), _stream())
        return quant.Fp8Act(q, s, x.shape, x.dtype), residual
    y = torch.empty_like(x)
    _ext.kernels().rms_norm(y.data_ptr(), x.data_ptr(), residual.data_ptr(), w.data_ptr(), x.numel() // h, h,
                            float(eps), _stream())
    return y, residual


def qkv_prep_(qkv: torch.Tensor, bias: Optional[torch.Tensor], q_w: Optional[torch.Tensor],
              k_w: Optional[torch.Tensor], hq: int, hkv: int, d: int, eps: float) -> torch.Tensor:
    """Qwen2 qkv bias / Qwen3 per-head q, k RMSNorm over ``d``, in place on the dense projection output
    ``qkv`` [T, (hq + 2 hkv) d] before RoPE (contract: ops/reference.py qkv_prep).  ``bias``
    [(hq + 2 hkv) d], ``q_w`` / ``k_w`` [d], each optional; head slots that none of them touches are
    neither read nor written.  One launch, nothing allocated: graph-capturable."""
    if qkv.dim() != 2 or qkv.shape[1] != (hq + 2 * hkv) * d:
        raise ValueError(f"qkv_prep_: qkv must be [T, {(hq + 2 * hkv) * d}], got {tuple(qkv.shape)}")
    for t, name, n in ((bias, "bias", (hq + 2 * hkv) * d), (q_w, "q_w", d), (k_w, "k_w", d)):
        if t is not None and (t.shape != (n,) or t.device != qkv.device):
            raise ValueError(f"qkv_prep_: {name} must be [{n}] on qkv's device")
    if not _gpu(qkv):
        return ref.qkv_prep(qkv, bias, q_w, k_w, hq, hkv, d, eps)
    _ck(qkv, "qkv_prep_.qkv")
    for t, name in ((bias, "bias"), (q_w, "q_w"), (k_w, "k_w")):
        if t is not None:
            _ck(t, "qkv_prep_." + name)
    if d not in (64, 128):
        raise ValueError(f"qkv_prep_: head_dim must be 64 or 128, got {d}")
    ptr = lambda t: 0 if t is None else t.data_ptr()
    _ext.kernels().qkv_prep(qkv.data_ptr(), ptr(bias), ptr(q_w), ptr(k_w), qkv.shape[0], hq, hkv, d, float(eps),
                            _stream())
    return qkv


def layer_norm(x, w, b, eps):
    # GPT-2 plumbing config only: torch path on both devices.
    return ref.layer_norm(x, w, b, eps)


def gelu_tanh(x):
    return ref.gelu_tanh(x)


# --------------------------------------------------------------- GEMM
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, defer: bool = False):
    """y = x @ w^T (+bias). w is [N, K].  ``defer`` (GPU): the result may come back as a
    :class:`gemm.SplitKPartial` for ``fused_add_rms_norm`` to reduce (or ``materialize()``).
    ``w`` may be a :class:`quant.Fp8Weight` (W8A8 e4m3 GEMM, no bias)."""
    if isinstance(w, quant.Fp8Weight):
        if bias is not None:
            raise ValueError("linear: fp8 weights take no bias")
        return quant.linear_fp8(x, w, defer=defer)
    if not _gpu(x):
        return ref.linear(x, w, bias)
    return gemm.linear(x, w, bias, defer=defer)


def linear_swiglu(x: torch.Tensor, w_gate_up: torch.Tensor) -> torch.Tensor:
    """silu(x @ Wg^T) * (x @ Wu^T), W = [Wg; Wu]; fused into the GEMM epilogue on the GPU (decode)."""
    if isinstance(w_gate_up, quant.Fp8Weight):
        return quant.linear_fp8(x, w_gate_up, swiglu=True)
    if _gpu(x):
        y = gemm.linear_swiglu(x, w_gate_up)
        if y is not None:                    # None: gemm.route found no fused kernel (GemmRoute.unfused)
            return y
    return silu_mul(linear(x, w_gate_up))


def add_(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a <- a + b (in place)."""
    if not _gpu(a):
        a.copy_((a.float() + b.float()).to(a.dtype))
        return a
    _ck(a, "add_.a")
    _ck(b, "add_.b")
    if a.shape != b.shape:
        raise ValueError("add_: shape mismatch")
    _ext.kernels().add_inplace(a.data_ptr(), b.data_ptr(), a.numel(), _stream())
    return a


# ------------------------------------------------------------ SwiGLU
def silu_mul(gu: torch.Tensor) -> torch.Tensor:
    if not _gpu(gu):
        return ref.silu_mul(gu)
    _ck(gu, "silu_mul.gu")
    t, two_i = gu.shape
    out = torch.empty(t, two_i // 2, dtype=gu.dtype, device=gu.device)
    _ext.kernels().silu_mul(out.data_ptr(), gu.data_ptr(), t, two_i // 2, _stream())
    return out


# ------------------------------------------------- K4 - K7: ops/attention.py
# (imported here, below the helpers it takes from this module)
from .attention import (MAX_DECODE_SPLITS, PF_MAX_CHUNKS, PF_SPLIT_MAX_PLAIN_WGS, PF_SPLIT_MAX_Q,  # noqa: E402,F401
                        PF_SPLIT_MIN_CHUNKS, PF_SPLIT_TARGET_WGS, PREFILL_SPLIT, PrefillRoute, decode_split_plan,
                        decode_workspace, paged_attention_decode, paged_attention_decode_rope,
                        paged_attention_prefill, paged_attention_prefill_rope, prefill_attn_version, prefill_route,
                        prefill_split_eligible, prefill_split_plan, rope_cache_append)


# ------------------------------------------------------------- K10
def argmax(logits: torch.Tensor) -> torch.Tensor:
    if not _gpu(logits):
        return ref.argmax(logits)
    if logits.dtype != torch.bfloat16:
        return logits.argmax(-1).to(torch.int32)
    if logits.stride(-1) != 1:
        raise ValueError("argmax: last dim must be contiguous")
    rows, v = logits.shape
    out = torch.empty(rows, dtype=torch.int32, device=logits.device)
    _ext.kernels().argmax(out.data_ptr(), logits.data_ptr(), rows, v, logits.stride(0), _stream())
    return out


SAMPLE_MAX_VOCAB = 131072      # csrc/kernels/sampler.hip: 16 groups of 8 entries per thread, 1024 threads
_host_sampler_warned = False


def _warn_host_sampler(logits: torch.Tensor, op: str = "sample_rows") -> None:
    """Once per process: GPU logits are about to be sampled by the host reference."""
    global _host_sampler_warned
    if not _host_sampler_warned:
        _host_sampler_warned = True
        import logging
        logging.getLogger("dllm.ops").warning(
            "%s: %s logits on %s take the host reference (knobs.fused_sampler=%s): the [B, V] logits are "
            "copied to the host every step, which synchronises the device and cannot be graph-captured",
            op, logits.dtype, logits.device, knobs.K.fused_sampler)


def sample_rows(logits: torch.Tensor, params: torch.Tensor, seeds: torch.Tensor, pos: torch.Tensor,
                uniforms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Seeded temperature / top-k / top-p sampling, one id per row (contract: ops/reference.py).

    logits [B, V]; params [B, 3] int32 (temperature * 1e4, top_k, top_p * 1e4); seeds [B] int64
    (the 64-bit seed's bit pattern); pos [B] int32 (index of the token being drawn); uniforms [B]
    float32 or None (test hook: replaces the Philox draw).  Every per-row value is read on the
    device: no host synchronisation, graph-capturable.  bf16 CUDA logits with a contiguous last dim
    (at most SAMPLE_MAX_VOCAB entries) take the HIP kernel; anything else, and everything with
    ``knobs.fused_sampler`` off, the reference -- numpy on the host, so GPU logits then cost a
    device-to-host copy and a synchronisation per step (logged once)."""
    if not (_gpu(logits) and logits.dtype == torch.bfloat16 and logits.stride(-1) == 1 and knobs.K.fused_sampler):
        if _gpu(logits):
            _warn_host_sampler(logits)
        return ref.sample_rows(logits, params, seeds, pos, uniforms)
    rows, v = logits.shape
    if v > SAMPLE_MAX_VOCAB:
        raise ValueError(f"sample_rows: vocab {v} exceeds the kernel's register-resident row of {SAMPLE_MAX_VOCAB}")
    dev = logits.device
    _ck(params, "sample_rows.params", torch.int32)
    _ck(seeds, "sample_rows.seeds", torch.int64)
    _ck(pos, "sample_rows.pos", torch.int32)
    if params.shape != (rows, 3) or seeds.shape != (rows,) or pos.shape != (rows,):
        raise ValueError(f"sample_rows: params / seeds / pos must be [{rows}, 3] / [{rows}] / [{rows}]")
    if uniforms is not None:
        _ck(uniforms, "sample_rows.uniforms", torch.float32)
        if uniforms.shape != (rows,):
            raise ValueError(f"sample_rows: uniforms must be [{rows}]")
    if any(t.device != dev for t in (params, seeds, pos) + (() if uniforms is None else (uniforms,))):
        raise ValueError("sample_rows: params, seeds, pos and uniforms must be on the logits' device")
    out = torch.empty(rows, dtype=torch.int32, device=dev)
    _ext.kernels().sample_rows(out.data_ptr(), logits.data_ptr(), rows, v, logits.stride(0), params.data_ptr(),
                               seeds.data_ptr(), pos.data_ptr(), 0 if uniforms is None else uniforms.data_ptr(),
                               _stream())
    return out


MAX_LOGPROBS = ref.MAX_LOGPROBS     # csrc/kernels/launchers.h kMaxLogprobs


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, want: torch.Tensor, n_max: int):
    """Log-probabilities of the model's distribution (contract: ops/reference.py token_logprobs).

    logits [B, V]; ids [B] int32 (the token each row chose); want [B] int32 (-1: the row is
    skipped, else how many of the most likely entries to report, at most ``n_max`` <=
    MAX_LOGPROBS) -> (chosen [B] float32, top_ids [B, n_max] int32, top_lp [B, n_max] float32).
    Every per-row value is read on the device.  bf16 CUDA logits with a contiguous last dim of at
    most SAMPLE_MAX_VOCAB entries take the HIP kernel; anything else, and everything with
    ``knobs.fused_sampler`` off, the host reference (GPU logits: logged once, as sample_rows)."""
    n_max = int(n_max)
    if not 0 <= n_max <= MAX_LOGPROBS:
        raise ValueError(f"token_logprobs: n_max must be in [0, {MAX_LOGPROBS}], got {n_max}")
    if logits.dim() != 2:
        raise ValueError("token_logprobs: logits must be [B, V]")
    rows, v = logits.shape
    _ck(ids, "token_logprobs.ids", torch.int32)
    _ck(want, "token_logprobs.want", torch.int32)
    if ids.shape != (rows,) or want.shape != (rows,):
        raise ValueError(f"token_logprobs: ids / want must be [{rows}] / [{rows}]")
    if ids.device != logits.device or want.device != logits.device:
        raise ValueError("token_logprobs: ids and want must be on the logits' device")
    if not (_gpu(logits) and logits.dtype == torch.bfloat16 and logits.stride(-1) == 1 and knobs.K.fused_sampler
            and v <= SAMPLE_MAX_VOCAB):
        if _gpu(logits):
            _warn_host_sampler(logits, "token_logprobs")
        return ref.token_logprobs(logits, ids, want, n_max)
    dev = logits.device
    chosen = torch.empty(rows, dtype=torch.float32, device=dev)
    top_ids = torch.empty(rows, n_max, dtype=torch.int32, device=dev)
    top_lp = torch.empty(rows, n_max, dtype=torch.float32, device=dev)
    _ext.kernels().token_logprobs(chosen.data_ptr(), top_ids.data_ptr(), top_lp.data_ptr(), logits.data_ptr(), rows, v,
                                  logits.stride(0), ids.data_ptr(), want.data_ptr(), n_max, _stream())
    return chosen, top_ids, top_lp


# ------------------------------------------------------------ logit processors
# Penalties, logit_bias and the min_tokens EOS ban (contract: ops/reference.py).  ``ls`` is an
# engine.logit_state.LogitState (or anything with its tensors): state [rows, pitch] int32, bias_n
# [rows] int32, bias_ids [rows, P] int32, bias_vals [rows, P] float32, and ``vocab``.
def _fused_processors(logits_like: torch.Tensor, vocab: int) -> bool:
    return _gpu(logits_like) and knobs.K.fused_sampler and vocab <= SAMPLE_MAX_VOCAB


def _ck_state(ls, op: str, procs: torch.Tensor, rows: int):
    _ck(ls.state, f"{op}.state", torch.int32)
    _ck(procs, f"{op}.procs", torch.int32)
    if procs.shape != (rows, ref.PROC_WORDS):
        raise ValueError(f"{op}: procs must be [{rows}, {ref.PROC_WORDS}]")
    if ls.state.dim() != 2 or ls.state.shape[1] % 8 or ls.state.shape[1] < ls.vocab:
        raise ValueError(f"{op}: state must be [rows, pitch], pitch a multiple of 8 covering the vocabulary")
    _ck(ls.bias_n, f"{op}.bias_n", torch.int32)
    _ck(ls.bias_ids, f"{op}.bias_ids", torch.int32)
    _ck(ls.bias_vals, f"{op}.bias_vals", torch.float32)
    n = ls.state.shape[0]
    if ls.bias_n.shape != (n,) or ls.bias_ids.dim() != 2 or ls.bias_ids.shape[0] != n \
            or ls.bias_vals.shape != ls.bias_ids.shape:
        raise ValueError(f"{op}: bias_n / bias_ids / bias_vals must be [{n}] / [{n}, P] / [{n}, P]")
    if any(t.device != ls.state.device for t in (procs, ls.bias_n, ls.bias_ids, ls.bias_vals)):
        raise ValueError(f"{op}: procs and the bias tensors must be on the state's device")


def logit_state_update(ls, ids: torch.Tensor, cu_seqlens: torch.Tensor, procs: torch.Tensor,
                       step_bias_cu: torch.Tensor, step_bias_ids: torch.Tensor, step_bias_vals: torch.Tensor) -> None:
    """A step's prefill chunks enter the state: ids [T] int32, cu_seqlens [B + 1] int32, procs
    [B, PROC_WORDS] int32 (rows with PROC_UPDATE and a state row take part; PROC_START is the
    position of the chunk's first token), step_bias_* the bias lists of the step (cu [B + 1], ids
    and float32 values [n]) that chunks starting at position 0 install."""
    rows = procs.shape[0]
    _ck_state(ls, "logit_state_update", procs, rows)
    _ck(ids, "logit_state_update.ids", torch.int32)
    _ck(cu_seqlens, "logit_state_update.cu_seqlens", torch.int32)
    _ck(step_bias_cu, "logit_state_update.step_bias_cu", torch.int32)
    _ck(step_bias_ids, "logit_state_update.step_bias_ids", torch.int32)
    _ck(step_bias_vals, "logit_state_update.step_bias_vals", torch.float32)
    if cu_seqlens.shape != (rows + 1,) or step_bias_cu.shape != (rows + 1,) \
            or step_bias_ids.shape != step_bias_vals.shape or step_bias_ids.dim() != 1:
        raise ValueError("logit_state_update: cu_seqlens / step_bias_cu must be [B + 1], the bias lists [n]")
    if any(t.device != ls.state.device for t in (ids, cu_seqlens, step_bias_cu, step_bias_ids, step_bias_vals)):
        raise ValueError("logit_state_update: every tensor must be on the state's device")
    if not _fused_processors(ls.state, ls.vocab):
        return ref.logit_state_update(ls.state, ls.vocab, ids, cu_seqlens, procs, ls.bias_n, ls.bias_ids,
                                      ls.bias_vals, step_bias_cu, step_bias_ids, step_bias_vals)
    _ext.kernels().logit_state_update(ls.state.data_ptr(), ls.state.shape[1], ls.state.shape[0], ls.vocab,
                                      ids.data_ptr(), cu_seqlens.data_ptr(), procs.data_ptr(), rows,
                                      ls.bias_n.data_ptr(), ls.bias_ids.data_ptr(), ls.bias_vals.data_ptr(),
                                      ls.bias_ids.shape[1], step_bias_cu.data_ptr(), step_bias_ids.data_ptr(),
                                      step_bias_vals.data_ptr(), _stream())


def apply_logit_processors(logits: torch.Tensor, ls, procs: torch.Tensor, seq_lens: torch.Tensor,
                           eos_id: int) -> torch.Tensor:
    """The processors on ``logits`` [B, V], in place, for the rows with PROC_SAMPLE and a state row;
    every other row is neither read nor written.  seq_lens [B] int32: a row draws output token
    number seq_lens - prompt_len, and ``eos_id`` (-1: none) is banned while that is < min_tokens.
    bf16 CUDA logits with a contiguous last dim of at most SAMPLE_MAX_VOCAB entries take the HIP
    kernel (with ``knobs.fused_sampler`` on); anything else the reference."""
    if logits.dim() != 2 or logits.shape[1] != ls.vocab:
        raise ValueError(f"apply_logit_processors: logits must be [B, {ls.vocab}]")
    rows, v = logits.shape
    _ck_state(ls, "apply_logit_processors", procs, rows)
    _ck(seq_lens, "apply_logit_processors.seq_lens", torch.int32)
    if seq_lens.shape != (rows,) or seq_lens.device != logits.device or ls.state.device != logits.device:
        raise ValueError("apply_logit_processors: seq_lens must be [B]; everything on the logits' device")
    eos_id = -1 if eos_id is None else int(eos_id)
    if not -1 <= eos_id < v:
        raise ValueError(f"apply_logit_processors: eos id {eos_id} outside the vocabulary")
    if not (_fused_processors(logits, v) and logits.dtype == torch.bfloat16 and logits.stride(-1) == 1
            and (rows <= 1 or logits.stride(0) >= v)):
        if _gpu(logits):
            _warn_host_sampler(logits, "apply_logit_processors")
        ref.apply_logit_processors(logits, ls.state, procs, seq_lens, eos_id, ls.bias_n, ls.bias_ids, ls.bias_vals)
        return logits
    _ext.kernels().apply_logit_processors(logits.data_ptr(), rows, v, max(logits.stride(0), v), ls.state.data_ptr(),
                                          ls.state.shape[1], ls.state.shape[0], procs.data_ptr(), seq_lens.data_ptr(),
                                          eos_id, ls.bias_n.data_ptr(), ls.bias_ids.data_ptr(),
                                          ls.bias_vals.data_ptr(), ls.bias_ids.shape[1], _stream())
    return logits


def logit_state_count(ls, ids: torch.Tensor, procs: torch.Tensor) -> None:
    """After sampling: ids [B] int32, the id each row drew; rows with PROC_SAMPLE and a state row
    add one to that id's count."""
    rows = procs.shape[0]
    _ck_state(ls, "logit_state_count", procs, rows)
    _ck(ids, "logit_state_count.ids", torch.int32)
    if ids.shape != (rows,) or ids.device != ls.state.device:
        raise ValueError(f"logit_state_count: ids must be [{rows}] on the state's device")
    if not _fused_processors(ls.state, ls.vocab):
        return ref.logit_state_count(ls.state, ls.vocab, ids, procs)
    _ext.kernels().logit_state_count(ls.state.data_ptr(), ls.state.shape[1], ls.state.shape[0], ls.vocab,
                                     ids.data_ptr(), procs.data_ptr(), rows, _stream())


# ------------------------------------------------------------ K11/K12
def moe_route(router_logits: torch.Tensor, top_k: int):
    from . import moe
    return moe.route(router_logits, top_k)


def moe_mlp(x, w_gate_up, w_down, topk_w, topk_ids):
    from . import moe
    return moe.mlp(x, w_gate_up, w_down, topk_w, topk_ids)


def moe_forward(x, w_router, w_gate_up, w_down, top_k: int, expert_offset: int = 0):
    """Full Mixtral sparse MLP: route + expert SwiGLU MLPs + weighted combine (``expert_offset``:
    the weights hold experts [offset, offset + E_local) -- expert parallelism, ops/moe.py)."""
    from . import moe
    return moe.forward(x, w_router, w_gate_up, w_down, top_k, expert_offset)
