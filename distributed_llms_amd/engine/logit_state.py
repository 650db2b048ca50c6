"""Per-request token statistics of the logit processors, on the device of the stage that samples.

Outputs of a running sequence live in the native batcher, and with lookahead decode the host has
not even seen the newest token when it builds the next step, so the counts the penalties need
cannot be shipped from the host every step.  They live here: one STATE ROW of ``pitch`` int32 words
per request that asks (``Sequence.state_row``, handed out by the Scheduler), word t = the output
count of token t | STATE_BIAS_BIT | STATE_PROMPT_BIT (ops/reference.py), plus the request's bias
list in small side tensors.  The kernels of csrc/kernels/logit_processors.hip keep a row current
(``ops.logit_state_update`` for prefill chunks, ``ops.logit_state_count`` for sampled ids) and
apply it (``ops.apply_logit_processors``); engine/sampler.py ``sample_step`` strings them around a
step's sampling.

Nothing is allocated until a step carries a processors section: 4 * pitch bytes per row (512 KB at
a vocabulary of 128,256) times ``HostBatch.state_rows``, the same number on every stage.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops
from ..ops.reference import MAX_LOGIT_BIAS, PROC_FLAGS, PROC_UPDATE

BIAS_PITCH = 304        # MAX_LOGIT_BIAS entries, rounded up to a multiple of 16 bytes


class LogitState:
    def __init__(self):
        self.vocab = 0
        self.state: Optional[torch.Tensor] = None        # [rows, pitch] int32
        self.bias_n: Optional[torch.Tensor] = None       # [rows] int32
        self.bias_ids: Optional[torch.Tensor] = None     # [rows, BIAS_PITCH] int32
        self.bias_vals: Optional[torch.Tensor] = None    # [rows, BIAS_PITCH] float32

    @property
    def allocated(self) -> bool:
        return self.state is not None

    def ensure(self, rows: int, vocab: int, device) -> "LogitState":
        """Allocate on first use (zero-filled; a row is reset by its request's first chunk before
        anything reads it)."""
        device = torch.device(device)
        if self.state is not None:
            if self.state.shape[0] != rows or self.vocab != vocab or self.state.device != device:
                raise ValueError(f"LogitState of {self.state.shape[0]} rows x {self.vocab} tokens on "
                                 f"{self.state.device} asked for {rows} x {vocab} on {device}")
            return self
        if rows < 1 or vocab < 1:
            raise ValueError("LogitState needs at least one row and one token")
        assert MAX_LOGIT_BIAS <= BIAS_PITCH
        self.vocab = int(vocab)
        pitch = -(-self.vocab // 8) * 8
        self.state = torch.zeros(rows, pitch, dtype=torch.int32, device=device)
        self.bias_n = torch.zeros(rows, dtype=torch.int32, device=device)
        self.bias_ids = torch.zeros(rows, BIAS_PITCH, dtype=torch.int32, device=device)
        self.bias_vals = torch.zeros(rows, BIAS_PITCH, dtype=torch.float32, device=device)
        if device.type == "cuda":
            # once: the fills above are behind us before another stream's first reset of a row
            torch.cuda.synchronize(device)
        return self


def stage_section(hb, device, upload) -> dict:
    """The step's processors section on ``device``, one upload ([procs | seq_lens | cu_seqlens |
    bias_cu | bias ids | bias values | chunk ids]; the tail from cu_seqlens on only when a chunk
    enters the state).  ``upload``: int32 numpy array -> device tensor."""
    b = hb.num_seqs
    update = bool((hb.procs[:, PROC_FLAGS] & PROC_UPDATE).any())
    parts = [hb.procs.reshape(-1), hb.seq_lens]
    if update:
        parts += [hb.cu_seqlens, hb.bias_cu, hb.bias_ids, hb.bias_vals, hb.ids]
    sizes = [int(p.shape[0]) for p in parts]
    t = upload(np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1) for p in parts]))
    views = torch.split(t, sizes)
    out = {"procs": views[0].view(b, -1), "seq_lens": views[1], "update": update}
    if update:
        out.update(cu_seqlens=views[2], bias_cu=views[3], bias_ids=views[4], bias_vals=views[5].view(torch.float32),
                   ids=views[6])
    return out
