"""Token sampling on the last stage.

Greedy rows use the argmax kernel (K10 tail) on bf16 logits.  With per-row seeds (every batch the
engines build) the rows with temperature > 0 go through ``ops.sample_rows``: one HIP kernel, a
stateless Philox draw per (seed, position), so a request's tokens do not depend on its batch, its
step or a preemption.  Without seeds the rows use softmax + top-k/top-p + multinomial in torch
(fp32, torch's generator).
"""
from __future__ import annotations

from typing import Optional, Sequence as Seq

import numpy as np
import torch

from .. import ops
from .logit_state import stage_section
from .sequence import MAX_LOGPROBS, split_seed


def sample(logits: torch.Tensor, temperatures: Optional[Seq[float]] = None, top_k: Optional[Seq[int]] = None,
           top_p: Optional[Seq[float]] = None, generator: Optional[torch.Generator] = None,
           seeds=None, positions=None) -> torch.Tensor:
    """logits [B, V] -> ids [B] int32 (device).  ``seeds`` [B, 2] int32 (low, high words) with
    ``positions`` [B] (index of the token each row draws): the seeded path."""
    if temperatures is None or all(t <= 0 for t in temperatures):
        return ops.argmax(logits)
    if seeds is not None:
        return _sample_seeded(logits, temperatures, top_k, top_p, seeds, positions)
    greedy = ops.argmax(logits)
    temps = torch.tensor([max(t, 1e-5) for t in temperatures], device=logits.device, dtype=torch.float32)
    lf = logits.float() / temps.unsqueeze(1)
    if top_k is not None and any(k > 0 for k in top_k):
        # one batched mask: row i keeps logits >= its k-th largest (k <= 0: every logit)
        kmax = min(max(top_k), lf.shape[1])
        vals, _ = torch.topk(lf, kmax, dim=-1)
        ks = torch.tensor(list(top_k), device=lf.device)
        thresh = vals.gather(1, (ks.clamp(1, kmax) - 1).unsqueeze(1))
        thresh = thresh.masked_fill((ks <= 0).unsqueeze(1), float("-inf"))
        lf = lf.masked_fill(lf < thresh, float("-inf"))
    probs = torch.softmax(lf, dim=-1)
    if top_p is not None and any(p < 1.0 for p in top_p):
        sp, si = torch.sort(probs, dim=-1, descending=True)
        cum = sp.cumsum(-1)
        tp = torch.tensor(list(top_p), device=logits.device).unsqueeze(1)
        mask = (cum - sp) > tp
        sp = sp.masked_fill(mask, 0.0)
        probs = torch.zeros_like(probs).scatter_(-1, si, sp)
        probs = probs / probs.sum(-1, keepdim=True)
    drawn = torch.multinomial(probs, 1, generator=generator).squeeze(1).to(torch.int32)
    is_greedy = torch.tensor([t <= 0 for t in temperatures], device=logits.device)
    return torch.where(is_greedy, greedy, drawn)


# pinned buffers per device: more than the uploads of the steps one slot keeps in flight (a step
# makes up to three: the sampler's parameters and, when a row asks, the logprobs counts and the
# processors section)
_STAGE_DEPTH = 8
_stages: dict = {}


def _stage(host: np.ndarray, device) -> torch.Tensor:
    """Upload ``host`` (int32) through a small ring of reused pinned buffers instead of pinning a
    fresh tensor every step.  A buffer is written again only after the copy that last read it has
    completed (its event; with the ring deeper than the steps in flight that wait is a no-op)."""
    ring = _stages.setdefault(torch.device(device), {"i": 0, "slots": [None] * _STAGE_DEPTH})
    i = ring["i"]
    ring["i"] = (i + 1) % _STAGE_DEPTH
    slot = ring["slots"][i]
    n = host.shape[0]
    if slot is None or slot[0].shape[0] < n:
        if slot is not None:
            slot[1].synchronize()
        slot = ring["slots"][i] = (torch.empty(max(n, 1536), dtype=torch.int32).pin_memory(), torch.cuda.Event())
    else:
        slot[1].synchronize()
    buf, ev = slot
    buf[:n].numpy()[:] = host
    dev = buf[:n].to(device, non_blocking=True)
    ev.record(torch.cuda.current_stream(device))
    return dev


def _sample_seeded(logits, temperatures, top_k, top_p, seeds, positions) -> torch.Tensor:
    """One staging buffer [params 3B | positions B | seeds 2B] int32, one (pinned, non-blocking on
    the GPU) copy; the seeds' offset of 4B words keeps them 8-byte aligned."""
    b = logits.shape[0]
    if positions is None:
        raise ValueError("sample: seeds need positions")
    host = np.empty(6 * b, dtype=np.int32)       # 6 int32 per row: 3 params, 1 position, 2 seed words
    par = host[:3 * b].reshape(b, 3)
    par[:, 0] = np.rint(np.asarray(temperatures, dtype=np.float64) * 1e4)
    par[:, 1] = 0 if top_k is None else np.asarray(top_k)
    par[:, 2] = 10000 if top_p is None else np.rint(np.asarray(top_p, dtype=np.float64) * 1e4)
    host[3 * b:4 * b] = np.asarray(positions)
    host[4 * b:] = np.asarray(seeds, dtype=np.int32).reshape(-1)
    if logits.is_cuda:
        t = _stage(host, logits.device)
    else:
        t = torch.from_numpy(host)
    return ops.sample_rows(logits, t[:3 * b].view(b, 3), t[4 * b:].view(torch.int64), t[3 * b:4 * b])


# ------------------------------------------------------------------ per-token log-probabilities
# A step in which some row asked for log-probabilities (``hb.logprobs`` is not None) answers with
# one int32 tensor, the step's IDS MESSAGE, instead of its B ids:
#     [ids B | chosen B (f32 bits) | top_ids B*N | top_lp B*N (f32 bits)],  N = max(hb.logprobs)
# With N = 0 the two top sections are empty; rows that did not ask hold the kernel's filler.  A
# step without an asking row sends its ids alone, as before.
def _top_n(hb) -> int:
    return max(0, int(hb.logprobs.max()))


def ids_message_len(hb) -> int:
    """int32 words the last stage answers a step with (both ends of a pipeline size by this)."""
    b = hb.num_seqs
    return b if hb.logprobs is None else b * (2 + 2 * _top_n(hb))


def max_ids_message_len(max_batch: int) -> int:
    """The longest ids message of a step of ``max_batch`` rows: every row asking for MAX_LOGPROBS
    entries.  Transports with fixed ids slots (RcclTransport's ``max_ids``) are sized by it."""
    return int(max_batch) * (2 + 2 * MAX_LOGPROBS)


def pack_ids_message(ids, chosen, top_ids, top_lp) -> torch.Tensor:
    return torch.cat([ids.to(torch.int32), chosen.view(torch.int32), top_ids.reshape(-1),
                      top_lp.reshape(-1).view(torch.int32)])


def unpack_ids_message(msg: np.ndarray, hb):
    """-> (ids [B] int32, logprobs): ``logprobs`` is None for a step without an asking row, else
    (chosen [B] float32, top_ids [B, N] int32, top_lp [B, N] float32), views of ``msg``."""
    b = hb.num_seqs
    msg = np.asarray(msg, dtype=np.int32)
    if msg.shape[0] != ids_message_len(hb):
        raise ValueError(f"ids message of {msg.shape[0]} words, expected {ids_message_len(hb)}")
    if hb.logprobs is None:
        return msg, None
    n = _top_n(hb)
    return msg[:b], (msg[b:2 * b].view(np.float32), msg[2 * b:(2 + n) * b].reshape(b, n),
                     msg[(2 + n) * b:].view(np.float32).reshape(b, n))


def sample_step(logits: torch.Tensor, hb, state=None, eos_id: Optional[int] = None):
    """Sample a step's rows -> (ids [B] int32, message).  ``message`` is None unless a row of the
    step asked for log-probabilities; then it is the ids message above: one more kernel
    (``ops.token_logprobs``) over the logits the ids were drawn from.

    A step with a processors section (``hb.procs``; ``state``: the caller's LogitState, ``eos_id``
    the id min_tokens bans) first brings the state rows of its prefill chunks up to date, then
    rewrites the asking rows of ``logits`` in place -- what argmax, the sampler and the
    log-probabilities then see -- and afterwards counts the ids those rows drew."""
    sec = None
    if hb.procs is not None:
        if state is None:
            raise ValueError("sample_step: the step carries logit processors but no LogitState was given")
        state.ensure(hb.state_rows, logits.shape[1], logits.device)
        sec = stage_section(hb, logits.device, (lambda a: _stage(a, logits.device)) if logits.is_cuda
                            else torch.from_numpy)
        if sec["update"]:
            ops.logit_state_update(state, sec["ids"], sec["cu_seqlens"], sec["procs"], sec["bias_cu"],
                                   sec["bias_ids"], sec["bias_vals"])
        ops.apply_logit_processors(logits, state, sec["procs"], sec["seq_lens"], -1 if eos_id is None else eos_id)
    ids = sample(logits, **hb.sampling_args())
    if sec is not None:
        ids = ids.to(torch.int32)
        ops.logit_state_count(state, ids, sec["procs"])
    if hb.logprobs is None:
        return ids, None
    want = np.ascontiguousarray(hb.logprobs, dtype=np.int32)
    want_t = _stage(want, logits.device) if logits.is_cuda else torch.from_numpy(want)
    ids = ids.to(torch.int32)
    return ids, pack_ids_message(ids, *ops.token_logprobs(logits, ids, want_t, _top_n(hb)))


def step_sampling_args(seqs) -> dict:
    """``sample`` arguments of a step over ``seqs``, as ``HostBatch.sampling_args()`` gives them
    for the step's batch.  A row draws the token at the index its context reaches in this step:
    the end of its chunk for a chunked prefill row, else its whole length (prefill and decode)."""
    temps = [s.params.temperature for s in seqs]
    if all(t <= 0 for t in temps):
        return {}
    return {"temperatures": temps, "top_k": [s.params.top_k for s in seqs],
            "top_p": [s.params.top_p for s in seqs],
            "seeds": np.array([split_seed(s.seed) for s in seqs], dtype=np.int32).reshape(len(seqs), 2),
            "positions": np.array([s.num_cached + s.chunk if s.chunk else s.total_len for s in seqs],
                                  dtype=np.int32)}
