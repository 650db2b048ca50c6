"""Multi-LoRA ops: the step's row plan and the batched shrink / expand (csrc/kernels/lora.hip).

Contract: ops/reference.py ``lora_apply``.  CPU tensors run that reference; CUDA tensors always go
to the HIP kernels (bf16 only) -- there is no eager fallback on the GPU.

The ROW PLAN is built on the host once per step and serves every layer and projection of it: the
token rows sorted stably by adapter slot and cut into tiles of 16 rows of one slot.  Rows without
an adapter (slot -1) are in no tile.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _ext
from . import reference as ref

TILE = ref.LORA_TILE


def max_tiles(rows: int, nslots: int) -> int:
    """Upper bound of a plan's tile count: every slot may leave one partly filled tile."""
    return -(-rows // TILE) + nslots


def row_plan(slots: np.ndarray, pad_tiles: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """slots [T] int (-1: no adapter) -> (tile_slot [nt] int32, tile_rows [nt * 16] int32, -1 =
    padding).  ``pad_tiles``: pad the plan with unused tiles (slot -1) to that many."""
    slots = np.asarray(slots, dtype=np.int32).reshape(-1)
    rows = np.flatnonzero(slots >= 0).astype(np.int32)
    rows = rows[np.argsort(slots[rows], kind="stable")]
    s = slots[rows]
    uniq, first, counts = np.unique(s, return_index=True, return_counts=True)
    tiles = -(-counts // TILE)
    nt = int(tiles.sum())
    n = nt if pad_tiles is None else int(pad_tiles)
    if n < nt:
        raise ValueError(f"row_plan: {nt} tiles do not fit the {n} planned for")
    tile_slot = np.full(n, -1, dtype=np.int32)
    tile_rows = np.full(n * TILE, -1, dtype=np.int32)
    t = 0
    for u, f, c, k in zip(uniq.tolist(), first.tolist(), counts.tolist(), tiles.tolist()):
        tile_slot[t:t + k] = u
        tile_rows[t * TILE:t * TILE + c] = rows[f:f + c]
        t += k
    return tile_slot, tile_rows


@dataclass
class LoraPlan:
    """A step's plan on the stage's device (BatchMeta.lora).  ``token_slot`` [T] int32 is what the
    CPU reference reads; ``tile_slot`` / ``tile_rows`` what the kernels read (``nt`` tiles)."""
    token_slot: torch.Tensor
    tile_slot: Optional[torch.Tensor] = None
    tile_rows: Optional[torch.Tensor] = None
    nt: int = 0


def make_plan(token_slots: np.ndarray, device) -> LoraPlan:
    """Upload the plan of a step whose token rows carry ``token_slots``."""
    dev = torch.device(device)
    token_slots = np.ascontiguousarray(token_slots, dtype=np.int32)
    if dev.type != "cuda":
        return LoraPlan(torch.from_numpy(token_slots))
    tile_slot, tile_rows = row_plan(token_slots)
    nt = tile_slot.shape[0]
    # one upload: [token_slot | tile_slot | tile_rows]
    t = token_slots.shape[0]
    buf = torch.from_numpy(np.concatenate([token_slots, tile_slot, tile_rows])).pin_memory().to(dev, non_blocking=True)
    return LoraPlan(buf[:t], buf[t:t + nt], buf[t + nt:], nt)


@dataclass
class LoraWeight:
    """The adapters of one projection, every slot in one tensor: a [slots, nslices * rp, K], b
    [slots, N, rp] (rp: the zero-padded rank), scale [slots] float32 (shared by the stage's
    projections), starts: first output column of every slice."""
    a: torch.Tensor
    b: torch.Tensor
    scale: torch.Tensor
    starts: Tuple[int, ...] = (0,)

    @property
    def nslots(self) -> int:
        return self.a.shape[0]

    @property
    def rp(self) -> int:
        return self.b.shape[-1]

    def nbytes(self) -> int:
        return self.a.numel() * self.a.element_size() + self.b.numel() * self.b.element_size()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ck(t: torch.Tensor, name: str, dtype, shape=None):
    if t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
        raise TypeError(f"lora.{name}: expected a contiguous CUDA {dtype} tensor, got {t.dtype} on {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"lora.{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def workspace_floats(k: int, nt: int, r: int) -> int:
    return _ext.kernels().lora_ksplit(k) * nt * TILE * r


def _ck_plan(plan: LoraPlan):
    _ck(plan.tile_slot, "tile_slot", torch.int32, (plan.nt,))
    _ck(plan.tile_rows, "tile_rows", torch.int32, (plan.nt * TILE,))


def shrink(x: torch.Tensor, w: LoraWeight, plan: LoraPlan, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The f32 K-slice partials of x A^T for the plan's rows: ws [ksplit, nt * 16, nslices * rp]."""
    t, k = x.shape
    s, r, _ = w.a.shape
    _ck(x, "x", torch.bfloat16)
    _ck(w.a, "a", torch.bfloat16, (s, r, k))
    _ck_plan(plan)
    need = workspace_floats(k, plan.nt, r)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=x.device)
    _ck(ws, "ws", torch.float32)
    _ext.kernels().lora_shrink(ws.data_ptr(), ws.numel(), x.data_ptr(), w.a.data_ptr(), plan.tile_slot.data_ptr(),
                               plan.tile_rows.data_ptr(), t, k, r, s, plan.nt, _stream())
    return ws


def expand(y: torch.Tensor, ws: torch.Tensor, k: int, w: LoraWeight, plan: LoraPlan) -> torch.Tensor:
    """y[t] <- bf16(y[t] + scale * (v[t] B^T)) in place for the plan's rows; ``ws``: shrink's
    partials of a [*, k] input.  ``y`` [T, N] may be a row-strided view (last dim contiguous)."""
    if y.dtype != torch.bfloat16 or not y.is_cuda or y.dim() != 2 or y.stride(1) != 1:
        raise TypeError("lora.y: expected a CUDA bfloat16 [T, N] tensor with a contiguous last dim")
    t, n = y.shape
    s, r, _ = w.a.shape
    rp = w.rp
    _ck(w.b, "b", torch.bfloat16, (s, n, rp))
    _ck(w.scale, "scale", torch.float32, (s,))
    _ck(ws, "ws", torch.float32)
    _ck_plan(plan)
    starts = tuple(w.starts)
    if not 1 <= len(starts) <= 3 or starts[0] != 0 or len(starts) * rp != r:
        raise ValueError("lora.expand: 1 to 3 slices, the first at column 0, one rp-row block of A each")
    off1 = starts[1] if len(starts) > 1 else n
    off2 = starts[2] if len(starts) > 2 else n
    _ext.kernels().lora_expand(y.data_ptr(), y.stride(0), ws.data_ptr(), ws.numel(), w.b.data_ptr(),
                               w.scale.data_ptr(), plan.tile_slot.data_ptr(), plan.tile_rows.data_ptr(), t, n, k, r,
                               rp, off1, off2, s, plan.nt, _stream())
    return y


def apply(y: torch.Tensor, x: torch.Tensor, w: LoraWeight, plan: LoraPlan) -> torch.Tensor:
    """The projection's dense output ``y`` [T, N] (= x W^T) gets its rows' adapter deltas, in place."""
    if not y.is_cuda:
        y.copy_(ref.lora_apply(y, x, plan.token_slot, w.a, w.b, w.scale, w.starts))
        return y
    if plan.nt == 0:
        return y
    if x.shape[0] != y.shape[0]:
        raise ValueError("lora.apply: x and y must have the same rows")
    return expand(y, shrink(x, w, plan), x.shape[1], w, plan)
