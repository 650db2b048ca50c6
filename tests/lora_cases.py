"""Inputs for the multi-LoRA kernels whose result is known to the last bit, their fp64 references and
the preconditions that make the comparison exact -- shared by tests/test_lora_gpu.py (GPU) and
tests/test_lora.py (CPU: the builders and preconditions themselves).

Everything is built on the CPU from a seed derived from the shape, so a case is the same tensors
wherever it is built.

Why the integer case is exact (contract: ops/reference.py lora_apply):
  * x holds integers in [-4, 4]; every row of A has at most 4 non-zero integers in [-8, 8], so
    |v| <= 4 * 4 * 8 = 128 <= 256: every v, and every partial sum towards it, is an integer that f32
    and bf16 hold exactly, in any summation order;
  * B holds integers in [-8, 8], so |d| <= 64 * 128 * 8 = 2^16: exact in f32 in any order;
  * scale is a power of two (1, 2, 4) and y0 a bf16-representable integer with |y0| <= 1024, so
    f32(y0) + scale * d is an integer below 2^24: exact in f32.  The only rounding is the final one to
    bf16, and the asserted shares of rounded (>= 0.05) and tied (>= 0.01) results pin its mode.
"""
import functools
from collections import namedtuple

import torch

from gemm_exact_cases import MIN_ROUNDED, MIN_TIES, bf16_shares, gen

BF16 = torch.bfloat16
F64 = torch.float64
NSLOTS = 3
SCALES = (1.0, 2.0, 4.0)
SLOT_PATTERN = (0, 1, 2, -1)           # row t carries SLOT_PATTERN[t % 4]: interleaved row by row
V_LIMIT = 256

LoraCase = namedtuple("LoraCase", "x a b scale slot y0 expected v starts rank rp rounded ties")


def rank_pad(rank):
    return 32 if rank <= 32 else 64


def row_slots(t):
    return torch.tensor([SLOT_PATTERN[i % 4] for i in range(t)], dtype=torch.int32)


def slice_starts(widths):
    return tuple(sum(widths[:i]) for i in range(len(widths)))


def reference64(x, a, b, scale, slot, y0, starts):
    """The contract in fp64: (y [T, N] fp64 before the final rounding, v [T, nslices * rp] fp64 after
    its bf16 rounding, absdot [T, N] = sum_j |v_j B_nj|).  Rows with slot -1 keep y0."""
    t, n = y0.shape
    rp = b.shape[-1]
    bounds = list(starts) + [n]
    y = y0.to(F64).clone()
    v_all = torch.zeros(t, a.shape[1], dtype=F64)
    absdot = torch.zeros(t, n, dtype=F64)
    for r in range(t):
        s = int(slot[r])
        if s < 0:
            continue
        v = (x[r].to(F64) @ a[s].to(F64).t()).to(BF16).to(F64)
        v_all[r] = v
        for i in range(len(bounds) - 1):
            c0, c1 = bounds[i], bounds[i + 1]
            bs = b[s, c0:c1].to(F64)
            y[r, c0:c1] += float(scale[s]) * (bs @ v[i * rp:(i + 1) * rp])
            absdot[r, c0:c1] = bs.abs() @ v[i * rp:(i + 1) * rp].abs()
    return y, v_all, absdot


@functools.lru_cache(maxsize=32)
def int_case(t, k, rank, widths, seed=0):
    """The exact integer case described in the module docstring; preconditions asserted here."""
    g = gen(t, k, rank, sum(widths), len(widths), seed)
    rp, nsl, n = rank_pad(rank), len(widths), sum(widths)
    starts = slice_starts(widths)
    x = torch.randint(-4, 5, (t, k), generator=g).to(F64)
    a = torch.zeros(NSLOTS, nsl * rp, k, dtype=F64)
    for s in range(NSLOTS):
        for i in range(nsl):
            for j in range(rank):
                cols = torch.randperm(k, generator=g)[:4]
                vals = torch.randint(1, 9, (4,), generator=g) * (torch.randint(0, 2, (4,), generator=g) * 2 - 1)
                a[s, i * rp + j, cols] = vals.to(F64)
    # asymmetric B: random integers, no structure shared between rows and columns
    b = torch.zeros(NSLOTS, n, rp, dtype=F64)
    b[:, :, :rank] = torch.randint(-8, 9, (NSLOTS, n, rank), generator=g).to(F64)
    y0 = torch.randint(-1024, 1025, (t, n), generator=g).to(F64).to(BF16)
    scale = torch.tensor(SCALES, dtype=torch.float32)
    assert all(float(s) == 2.0 ** round(float(torch.log2(s))) for s in scale), "scale must be a power of two"
    slot = row_slots(t)
    y, v, _ = reference64(x, a, b, scale, slot, y0, starts)
    # every v exactly representable in bf16 (the rounding inside reference64 changed nothing)
    raw = torch.stack([x[r] @ a[max(int(slot[r]), 0)].t() for r in range(t)])
    live = slot >= 0
    assert torch.equal(raw[live], v[live]) and v.abs().max().item() <= V_LIMIT, "v must be exact in bf16"
    # every partial sum exact in f32: bounded by the sum of magnitudes
    assert (x.abs() @ a.abs().amax(0).t()).max().item() < 2 ** 24
    assert y.abs().max().item() < 2 ** 24 and torch.equal(y, y.round())
    rounded, ties = bf16_shares(y[live])
    assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, (t, k, rank, widths, rounded, ties)
    return LoraCase(x.to(BF16), a.to(BF16), b.to(BF16), scale, slot, y0, y.to(BF16), v, starts, rank, rp,
                    rounded, ties)


@functools.lru_cache(maxsize=8)
def random_case(t, k, rank, widths, seed=0):
    """Random bf16 inputs; ``expected`` is the fp64 evaluation of the contract before the final
    rounding and ``bound`` (in place of rounded / ties: the per-element bound and None) is DERIVED:
    half a bf16 ulp of the result, plus 2^-8 * scale * sum_j |v_j B_nj| for one-ulp differences in
    v caused by the summation order, plus 2^-18 of the summed magnitudes for the f32 arithmetic of
    the expand (at most 64 + 2 roundings of 2^-24 each)."""
    g = gen(t, k, rank, sum(widths), len(widths), seed, 991)
    rp, nsl, n = rank_pad(rank), len(widths), sum(widths)
    starts = slice_starts(widths)
    x = torch.randn(t, k, generator=g).to(BF16)
    a = torch.zeros(NSLOTS, nsl * rp, k)
    for i in range(nsl):
        a[:, i * rp:i * rp + rank] = torch.randn(NSLOTS, rank, k, generator=g) / k ** 0.5
    b = torch.zeros(NSLOTS, n, rp)
    b[:, :, :rank] = torch.randn(NSLOTS, n, rank, generator=g)
    a, b = a.to(BF16), b.to(BF16)
    y0 = torch.randn(t, n, generator=g).to(BF16)
    scale = torch.tensor((0.5, 2.0, 1.375), dtype=torch.float32)
    slot = row_slots(t)
    y, v, absdot = reference64(x, a, b, scale, slot, y0, starts)
    return LoraCase(x, a, b, scale, slot, y0, y, v, starts, rank, rp, derived_bound(y, y0, scale, slot, absdot), None)


def derived_bound(y, y0, scale, slot, absdot):
    """The per-element bound of random_case's docstring (0 for rows without an adapter)."""
    sc = torch.tensor([float(scale[int(s)]) if s >= 0 else 0.0 for s in slot], dtype=F64)[:, None]
    t2 = 2.0 ** -8 * sc * absdot
    t3 = 2.0 ** -18 * (y0.to(F64).abs() + sc * absdot)
    mag = (y.abs() + t2 + t3).clamp(min=2.0 ** -126)
    half_ulp = torch.pow(torch.tensor(2.0, dtype=F64), torch.floor(torch.log2(mag)) - 8)
    bound = half_ulp + t2 + t3
    bound[slot < 0] = 0.0
    return bound


@functools.lru_cache(maxsize=4)
def needle_case(t, k, rank, n, seed=0):
    """Every slot's B is zero except one column unique to the slot: the delta can appear only in the
    rows of that slot and only in that column.  ``rounded``: the needle column of every slot;
    ``ties``: the derived bound (random_case).  Asserted here: the delta is visible in bf16 in every
    adapter row, with room for the bound."""
    c = random_case(t, k, rank, (n,), seed)
    g = gen(t, k, rank, n, seed, 5)
    cols = torch.randperm(n, generator=g)[:NSLOTS]
    b = torch.zeros_like(c.b)
    for s in range(NSLOTS):
        b[s, cols[s], :rank] = (torch.randint(1, 4, (rank,), generator=g).to(BF16))
    y, v, absdot = reference64(c.x, c.a, b, c.scale, c.slot, c.y0, c.starts)
    bound = derived_bound(y, c.y0, c.scale, c.slot, absdot)
    for r in range(t):
        s = int(c.slot[r])
        if s >= 0:
            col = int(cols[s])
            y0 = float(c.y0[r, col])
            gap = 2.0 ** (torch.floor(torch.log2(torch.tensor(max(abs(y0), 2.0 ** -126)))).item() - 7)   # one bf16 ulp of y0
            assert abs(float(y[r, col]) - y0) > float(bound[r, col]) + gap, (r, col)
    return c._replace(b=b, expected=y, v=v, rounded=cols, ties=bound)
