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
from . import gemm, int4, lora, quant
from . import reference as ref

__all__ = [
    "embedding", "rms_norm", "fused_add_rms_norm", "layer_norm", "linear", "silu_mul",
    "gelu_tanh", "rope_cache_append", "paged_attention_decode", "paged_attention_prefill",
    "argmax", "add_", "moe_route", "moe_mlp", "decode_split_plan", "paged_attention_decode_rope",
    "paged_attention_prefill_rope", "sample_rows", "token_logprobs", "lm_head_logprobs", "lm_head_ranges",
    "logit_state_update",
    "apply_logit_processors", "logit_state_count", "prefill_split_plan", "prefill_split_eligible", "qkv_prep_",
    "quantize_layers",
]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ck(t: torch.Tensor, name: str, dtype=torch.bfloat16, shape=None, device=None):
    """``t`` is a contiguous ``dtype`` tensor -- of ``shape`` (an extent of None: any) and on ``device``, if given."""
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and t.shape != shape and (t.dim() != len(shape) or
                                                   any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise ValueError(f"{name}: must be {list(shape)} (None: any extent), got {list(t.shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: must be on {device}, is on {t.device}")


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
    ``w`` may be a quantized weight (:func:`quantize_layers`), which then runs its own ``linear()``: a
    :class:`quant.Fp8Weight` (W8A8 e4m3 GEMM, no bias) or an :class:`int4.Int4Weight` (W4A16, no bias, always a
    dense result)."""
    if not isinstance(w, torch.Tensor):          # a quantized weight runs its own GEMM
        return w.linear(x, bias, defer)
    if not _gpu(x):
        return ref.linear(x, w, bias)
    return gemm.linear(x, w, bias, defer=defer)


def linear_swiglu(x: torch.Tensor, w_gate_up: torch.Tensor) -> torch.Tensor:
    """silu(x @ Wg^T) * (x @ Wu^T), W = [Wg; Wu]; fused into the GEMM epilogue on the GPU (decode)."""
    if not isinstance(w_gate_up, torch.Tensor):
        return w_gate_up.linear(x, swiglu=True)
    if _gpu(x):
        y = gemm.linear_swiglu(x, w_gate_up)
        if y is not None:                    # None: gemm.route found no fused kernel (GemmRoute.unfused)
            return y
    return silu_mul(linear(x, w_gate_up))


QUANT_MODULES = {"fp8": quant, "int4": int4}      # EngineConfig.quant -> the module of its weight format


def quantize_layers(layers, mode: str) -> int:
    """Replace the dense projections (quant.QUANT_KEYS; fp8: the MoE expert stacks too) of every layer dict by
    ``mode``'s weight objects, in place; returns how many were converted.  A quantized weight offers ``shape /
    device / dtype / numel() / nbytes() / dequantize()``, ``takes_fp8_act`` and the ``linear()`` that
    :func:`linear` / :func:`linear_swiglu` hand over to."""
    if mode not in QUANT_MODULES:
        raise ValueError(f"unknown quantization {mode!r} (none, fp8, int4)")
    mod = QUANT_MODULES[mode]
    n = mod.quantize_layers(layers, quant.QUANT_KEYS)
    if not n and getattr(mod, "NOTHING_CONVERTED", None):
        raise ValueError(mod.NOTHING_CONVERTED)
    return n


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
                        PF_SPLIT_MIN_CHUNKS, PF_SPLIT_TARGET_WGS, PREFILL_SPLIT, PREFILL_WINDOW, PrefillRoute,
                        decode_split_plan, decode_window_plan, decode_workspace, paged_attention_decode,
                        paged_attention_decode_rope, paged_attention_prefill, paged_attention_prefill_rope,
                        prefill_attn_version, prefill_route, prefill_split_eligible, prefill_split_plan,
                        prefill_window_max, rope_cache_append)


# ------------------------------------- K10 and the sampling stage: ops/sampling.py
from .sampling import (MAX_LOGPROBS, SAMPLE_MAX_VOCAB, apply_logit_processors, argmax, lm_head_logprobs,  # noqa: E402,F401
                       lm_head_ranges, logit_state_count, logit_state_update, sample_rows, token_logprobs)


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
