"""The sampling stage on the host (csrc/kernels/sampler.hip, logit_processors.hip, lm_head_logprobs.hip and
norm_elementwise.hip's argmax): which of the HIP kernel and the reference an op takes -- decided once, by
:func:`route` -- and the wrappers (their argument check is ops._ck)."""
from __future__ import annotations

import logging
from typing import Optional

import torch

from .. import _ext, knobs
from . import _ck, _gpu, _stream, gemm
from . import reference as ref

SAMPLE_MAX_VOCAB = 131072      # csrc/kernels/sampler.hip: 16 groups of 8 entries per thread, 1024 threads
MAX_LOGPROBS = ref.MAX_LOGPROBS     # csrc/kernels/launchers.h kMaxLogprobs
_host_sampler_warned = False        # the "reference-warn" warning is logged once per process


def route(op: str, *, is_cuda: bool, dtype, unit_stride: bool, row_stride: int, rows: int, vocab: int,
          fused: bool) -> str:
    """What ``op`` does with its deciding tensor: "kernel" (HIP), "reference" (ops/reference.py) or "reference-warn"
    (GPU logits take the host reference, a copy and a synchronisation per step; a warning is logged).  That tensor
    is the logits [rows, vocab]; for the two state ops ``ls.state`` with ``vocab = ls.vocab``; for lm_head_logprobs
    ``x`` [rows, K] with ``vocab = w.shape[0]``, ``unit_stride`` for "x is contiguous" and ``dtype`` None if w's
    differs.  ``fused``: knobs.fused_sampler.  Today's rules, differences included (docs/DESIGN.md lists those):

        op                      the kernel, on a CUDA tensor, needs               else
        argmax                  bf16                                              reference (torch on the device)
        sample_rows             bf16, unit stride, fused                          reference, CUDA: warn
        token_logprobs          bf16, unit stride, fused, fits                    reference, CUDA: warn
        apply_logit_processors  bf16, unit stride, fused, fits, rows apart        reference, CUDA: warn
        logit_state_update      fused, fits                                       reference
        logit_state_count       fused, fits                                       reference
        lm_head_logprobs        bf16, fused                                       reference
    fits: vocab <= SAMPLE_MAX_VOCAB; rows apart: rows <= 1 or row_stride >= vocab (the kernel writes them in place).
    ValueError on the way to the kernel: argmax and lm_head_logprobs without unit stride, sample_rows without fits."""
    bf16, fits = dtype == torch.bfloat16, vocab <= SAMPLE_MAX_VOCAB
    needs = {"argmax": bf16,
             "sample_rows": bf16 and unit_stride and fused,
             "token_logprobs": bf16 and unit_stride and fused and fits,
             "apply_logit_processors": bf16 and unit_stride and fused and fits and (rows <= 1 or row_stride >= vocab),
             "logit_state_update": fused and fits,
             "logit_state_count": fused and fits,
             "lm_head_logprobs": bf16 and fused}[op]
    if not (is_cuda and needs):
        warns = is_cuda and op in ("sample_rows", "token_logprobs", "apply_logit_processors")
        return "reference-warn" if warns else "reference"
    if op == "argmax" and not unit_stride:
        raise ValueError("argmax: last dim must be contiguous")
    if op == "lm_head_logprobs" and not unit_stride:
        raise ValueError("lm_head_logprobs.x: must be contiguous")
    if op == "sample_rows" and not fits:
        raise ValueError(f"sample_rows: vocab {vocab} exceeds the kernel's register-resident row of {SAMPLE_MAX_VOCAB}")
    return "kernel"


def _takes_kernel(op: str, t: torch.Tensor, vocab: int) -> bool:
    """:func:`route` for ``op`` with the deciding tensor ``t`` [rows, *]; logs the warning."""
    global _host_sampler_warned
    r = route(op, is_cuda=_gpu(t), dtype=t.dtype, unit_stride=t.stride(-1) == 1, row_stride=t.stride(0),
              rows=t.shape[0], vocab=vocab, fused=bool(knobs.K.fused_sampler))
    if r == "reference-warn" and not _host_sampler_warned:
        _host_sampler_warned = True
        logging.getLogger("dllm.ops").warning(
            "%s: %s logits on %s take the host reference (knobs.fused_sampler=%s): the [B, V] logits are "
            "copied to the host every step, which synchronises the device and cannot be graph-captured",
            op, t.dtype, t.device, knobs.K.fused_sampler)
    return r == "kernel"


def argmax(logits: torch.Tensor) -> torch.Tensor:
    if not _takes_kernel("argmax", logits, logits.shape[-1]):
        return ref.argmax(logits)
    rows, v = logits.shape
    out = torch.empty(rows, dtype=torch.int32, device=logits.device)
    _ext.kernels().argmax(out.data_ptr(), logits.data_ptr(), rows, v, logits.stride(0), _stream())
    return out


def sample_rows(logits: torch.Tensor, params: torch.Tensor, seeds: torch.Tensor, pos: torch.Tensor,
                uniforms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Seeded temperature / top-k / top-p sampling, one id per row (contract: ops/reference.py).

    logits [B, V]; params [B, 3] int32 (temperature * 1e4, top_k, top_p * 1e4); seeds [B] int64
    (the 64-bit seed's bit pattern); pos [B] int32 (index of the token being drawn); uniforms [B]
    float32 or None (test hook: replaces the Philox draw).  Every per-row value is read on the
    device: no host synchronisation, graph-capturable.  Kernel or reference (numpy on the host): :func:`route`."""
    if not _takes_kernel("sample_rows", logits, logits.shape[-1]):
        return ref.sample_rows(logits, params, seeds, pos, uniforms)
    (rows, v), dev = logits.shape, logits.device
    _ck(params, "sample_rows.params", torch.int32, (rows, 3), dev)
    _ck(seeds, "sample_rows.seeds", torch.int64, (rows,), dev)
    _ck(pos, "sample_rows.pos", torch.int32, (rows,), dev)
    if uniforms is not None:
        _ck(uniforms, "sample_rows.uniforms", torch.float32, (rows,), dev)
    out = torch.empty(rows, dtype=torch.int32, device=dev)
    _ext.kernels().sample_rows(out.data_ptr(), logits.data_ptr(), rows, v, logits.stride(0), params.data_ptr(),
                               seeds.data_ptr(), pos.data_ptr(), 0 if uniforms is None else uniforms.data_ptr(),
                               _stream())
    return out


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, want: torch.Tensor, n_max: int):
    """Log-probabilities of the model's distribution (contract: ops/reference.py token_logprobs).

    logits [B, V]; ids [B] int32 (the token each row chose); want [B] int32 (-1: the row is
    skipped, else how many of the most likely entries to report, at most ``n_max`` <=
    MAX_LOGPROBS) -> (chosen [B] float32, top_ids [B, n_max] int32, top_lp [B, n_max] float32).
    Every per-row value is read on the device.  Kernel or host reference: :func:`route`."""
    n_max = int(n_max)
    if not 0 <= n_max <= MAX_LOGPROBS:
        raise ValueError(f"token_logprobs: n_max must be in [0, {MAX_LOGPROBS}], got {n_max}")
    if logits.dim() != 2:
        raise ValueError("token_logprobs: logits must be [B, V]")
    (rows, v), dev = logits.shape, logits.device
    _ck(ids, "token_logprobs.ids", torch.int32, (rows,), dev)
    _ck(want, "token_logprobs.want", torch.int32, (rows,), dev)
    if not _takes_kernel("token_logprobs", logits, v):
        return ref.token_logprobs(logits, ids, want, n_max)
    chosen = torch.empty(rows, dtype=torch.float32, device=dev)
    top_ids = torch.empty(rows, n_max, dtype=torch.int32, device=dev)
    top_lp = torch.empty(rows, n_max, dtype=torch.float32, device=dev)
    _ext.kernels().token_logprobs(chosen.data_ptr(), top_ids.data_ptr(), top_lp.data_ptr(), logits.data_ptr(), rows, v,
                                  logits.stride(0), ids.data_ptr(), want.data_ptr(), n_max, _stream())
    return chosen, top_ids, top_lp


def lm_head_ranges(t: int, v: int, cus: int = 256, comm_cus: Optional[int] = None) -> int:
    """Vocabulary ranges S of the fused LM-head log-likelihood kernel: its grid is ceil(T / 256) row tiles x S,
    about one workgroup per CU that no comm kernel may hold (ops/gemm.py), a range at least one 256-column tile."""
    comm = gemm.comm_cus() if comm_cus is None else comm_cus
    return max(1, min(-(-v // 256), (cus - comm) // -(-t // 256)))


def lm_head_logprobs(x: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, ranges: int = 0) -> torch.Tensor:
    """Log-probability the LM head gives each row's target token (contract: ops/reference.py lm_head_logprobs):
    log_softmax(bf16(x w^T))[i, targets[i]] with linear, log-softmax and gather fused -- no [T, V] logits exist.

    x [T, K]; w [V, K]; targets [T] int32 (negative: the row is skipped and gets 0.0) -> float32 [T].  Kernel
    (csrc/kernels/lm_head_logprobs.hip: K % 64 == 0, any T and V, partial triples in the per-stream GEMM workspace,
    every value read on the device, graph-capturable, the same bits on every launch) or reference: :func:`route`.
    The reference also refuses a target >= V.  The kernel cannot (it reads targets on the device only) and gives
    such a row -inf: a caller that does not know its targets are below V checks them on the host first (the engine's
    are prompt tokens, validated against the vocabulary by the embedding path).  ``ranges``: the kernel's vocabulary
    ranges (0: :func:`lm_head_ranges`)."""
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or w.device != x.device:
        raise ValueError(f"lm_head_logprobs: x [T, K], w [V, K] on x's device, got {tuple(x.shape)}, {tuple(w.shape)}")
    (t, k), v = x.shape, w.shape[0]
    _ck(targets, "lm_head_logprobs.targets", torch.int32, (t,), x.device)
    if t == 0:
        return torch.empty(0, dtype=torch.float32, device=x.device)
    if route("lm_head_logprobs", is_cuda=_gpu(x), dtype=x.dtype if w.dtype == x.dtype else None,
             unit_stride=x.is_contiguous(), row_stride=x.stride(0), rows=t, vocab=v,
             fused=bool(knobs.K.fused_sampler)) != "kernel":
        return ref.lm_head_logprobs(x, w, targets)
    _ck(w, "lm_head_logprobs.w")
    if k % 64 or k < 64 or t * k * 2 >= 1 << 32 or v * k * 2 >= 1 << 32:
        raise ValueError("lm_head_logprobs: the kernel needs K % 64 == 0 and operands below 4 GiB")
    s = int(ranges) or lm_head_ranges(t, v, gemm._cus(x.device))
    if not 1 <= s <= -(-v // 256):
        raise ValueError(f"lm_head_logprobs: ranges must be in [1, {-(-v // 256)}], got {s}")
    ws = gemm._workspace(x.device)
    need = t * _ext.kernels().LM_HEAD_WAVES * s * 3       # (m, l, target logit) per row, range and wave
    if need > ws.numel():
        raise ValueError(f"lm_head_logprobs: {t} rows x {s} ranges need {need} workspace floats, "
                         f"the pool holds {ws.numel()}; score the rows in slices")
    out = torch.empty(t, dtype=torch.float32, device=x.device)
    _ext.kernels().lm_head_logprobs(out.data_ptr(), x.data_ptr(), w.data_ptr(), targets.data_ptr(), ws.data_ptr(),
                                    ws.numel(), t, v, k, s, _stream())
    return out


# ------------------------------------------------------------ logit processors
# Penalties, logit_bias and the min_tokens EOS ban (contract: ops/reference.py).  ``ls`` is an
# engine.logit_state.LogitState (or anything with its tensors): state [rows, pitch] int32, bias_n
# [rows] int32, bias_ids [rows, P] int32, bias_vals [rows, P] float32, and ``vocab``.
def _ck_state(ls, op: str, procs: torch.Tensor, rows: int, device=None):
    _ck(ls.state, f"{op}.state", torch.int32, (None, None), device)
    (n, pitch), dev = ls.state.shape, ls.state.device
    if pitch % 8 or pitch < ls.vocab:
        raise ValueError(f"{op}: state must be [rows, pitch], pitch a multiple of 8 covering the vocabulary")
    _ck(procs, f"{op}.procs", torch.int32, (rows, ref.PROC_WORDS), dev)
    _ck(ls.bias_n, f"{op}.bias_n", torch.int32, (n,), dev)
    _ck(ls.bias_ids, f"{op}.bias_ids", torch.int32, (n, None), dev)
    _ck(ls.bias_vals, f"{op}.bias_vals", torch.float32, tuple(ls.bias_ids.shape), dev)


def logit_state_update(ls, ids: torch.Tensor, cu_seqlens: torch.Tensor, procs: torch.Tensor,
                       step_bias_cu: torch.Tensor, step_bias_ids: torch.Tensor, step_bias_vals: torch.Tensor) -> None:
    """A step's prefill chunks enter the state: ids [T] int32, cu_seqlens [B + 1] int32, procs
    [B, PROC_WORDS] int32 (rows with PROC_UPDATE and a state row take part; PROC_START is the
    position of the chunk's first token), step_bias_* the bias lists of the step (cu [B + 1], ids
    and float32 values [n]) that chunks starting at position 0 install."""
    op, rows, dev = "logit_state_update", procs.shape[0], ls.state.device
    _ck_state(ls, op, procs, rows)
    _ck(ids, f"{op}.ids", torch.int32, None, dev)
    _ck(cu_seqlens, f"{op}.cu_seqlens", torch.int32, (rows + 1,), dev)
    _ck(step_bias_cu, f"{op}.step_bias_cu", torch.int32, (rows + 1,), dev)
    _ck(step_bias_ids, f"{op}.step_bias_ids", torch.int32, (None,), dev)
    _ck(step_bias_vals, f"{op}.step_bias_vals", torch.float32, tuple(step_bias_ids.shape), dev)
    if not _takes_kernel(op, ls.state, ls.vocab):
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
    Kernel or reference: :func:`route`."""
    if logits.dim() != 2 or logits.shape[1] != ls.vocab:
        raise ValueError(f"apply_logit_processors: logits must be [B, {ls.vocab}]")
    rows, v = logits.shape
    _ck_state(ls, "apply_logit_processors", procs, rows, logits.device)
    _ck(seq_lens, "apply_logit_processors.seq_lens", torch.int32, (rows,), logits.device)
    eos_id = -1 if eos_id is None else int(eos_id)
    if not -1 <= eos_id < v:
        raise ValueError(f"apply_logit_processors: eos id {eos_id} outside the vocabulary")
    if not _takes_kernel("apply_logit_processors", logits, v):
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
    _ck(ids, "logit_state_count.ids", torch.int32, (rows,), ls.state.device)
    if not _takes_kernel("logit_state_count", ls.state, ls.vocab):
        return ref.logit_state_count(ls.state, ls.vocab, ids, procs)
    _ext.kernels().logit_state_count(ls.state.data_ptr(), ls.state.shape[1], ls.state.shape[0], ls.vocab,
                                     ids.data_ptr(), procs.data_ptr(), rows, _stream())
