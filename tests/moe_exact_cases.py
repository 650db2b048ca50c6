"""Hand-built MoE routings and exactly representable operands for tests/test_moe_exact.py (GPU),
checked on the CPU by tests/test_exact_cases.py.  See test_moe_exact.py's docstring."""
import functools
from collections import namedtuple

import torch

from gemm_exact_cases import BF16, F64, gen, bf16_shares, SWIGLU_MAX_SUM

Routing = namedtuple("Routing", "counts offsets gather inv slot_expert t top_k slots")
MoeInt = namedtuple("MoeInt", "x w expected rounded ties")
MoeSwi = namedtuple("MoeSwi", "x w ref")
Combine = namedtuple("Combine", "ys topk_w inv exact")
RouteCase = namedtuple("RouteCase", "logits ids idle rx rw")

# (per-expert counts, top_k): T = sum(counts) / top_k tokens, each top_k times in ``gather``
ROUTINGS = [
    ((0, 1, 63, 64, 65, 0, 255, 257), 3),          # empty experts, every 64-row tile edge; T = 235
    ((0, 0, 0, 130, 0, 0, 0, 0), 2),               # all rows in one expert
    ((300, 0, 256, 1, 511, 0, 0, 212), 2),         # 256-row tiles end inside a segment (gemm_pp_moe)
]
# (n, k) of mode 0 and (inter, k) of mode 1, by [dims][gathered]: h, i in {256, 512} on both sides
INT_DIMS = [{True: (512, 256), False: (256, 512)}, {True: (256, 512), False: (512, 256)}]
SWIGLU_DIMS = [{True: (256, 256), False: (128, 512)}, {True: (512, 512), False: (256, 256)}]
COMBINE_CASES = [(t, k) for t in (1, 7, 300) for k in (1, 2)]


@functools.lru_cache(maxsize=8)
def routing(counts, top_k):
    """counts -> offsets (exclusive prefix sum, offsets[E] = slots), gather (slot -> token: a random
    permutation of every token top_k times), inv ((t, j) -> slot) and the expert owning each slot."""
    e = len(counts)
    slots = sum(counts)
    assert slots % top_k == 0
    t = slots // top_k
    g = gen(slots, top_k, e, 5)
    gather = torch.arange(t).repeat_interleave(top_k)[torch.randperm(slots, generator=g)].int()
    offsets = torch.zeros(e + 1, dtype=torch.int32)
    offsets[1:] = torch.tensor(counts).cumsum(0)
    slot_expert = torch.repeat_interleave(torch.arange(e), torch.tensor(counts)).int()
    # inv[t * top_k + j] = the j-th slot (in slot order) holding token t
    inv = torch.sort(gather.long(), stable=True).indices.int()
    return Routing(torch.tensor(counts, dtype=torch.int32), offsets, gather, inv, slot_expert, t, top_k, slots)


@functools.lru_cache(maxsize=8)
def moe_int_case(counts, top_k, n, k, gathered, r=8):
    """Integer x ([T, k] when gathered through ``gather``, else [slots, k]) and per-expert integer
    w [E, n, k], all different; expected[slot] = bf16(x_row(slot) @ w[expert(slot)]^T) from fp64."""
    assert k * r * r < 2 ** 24
    rt = routing(counts, top_k)
    g = gen(rt.slots, n, k, int(gathered), 9)
    x = torch.randint(-r, r + 1, (rt.t if gathered else rt.slots, k), generator=g).to(F64)
    w = torch.randint(-r, r + 1, (len(counts), n, k), generator=g).to(F64)
    xs = x[rt.gather.long()] if gathered else x
    y = torch.empty(rt.slots, n, dtype=F64)
    for e in range(len(counts)):
        a, b = rt.offsets[e].item(), rt.offsets[e + 1].item()
        y[a:b] = xs[a:b] @ w[e].t()
    rounded, ties = bf16_shares(y)
    assert rounded >= 0.05 and ties >= 0.01, (rounded, ties)
    return MoeInt(x.to(BF16), w.to(BF16), y.to(BF16), rounded, ties)


@functools.lru_cache(maxsize=8)
def moe_swiglu_case(counts, top_k, inter, k, gathered):
    """Ternary x, per-expert ternary x 2^-6 w [E, 2 inter, k] (part E of test_gemm_exact.py);
    ref[slot] = silu(g) u in fp64."""
    rt = routing(counts, top_k)
    g = gen(rt.slots, inter, k, int(gathered), 11)
    x = torch.randint(-1, 2, (rt.t if gathered else rt.slots, k), generator=g).to(F64)
    w = torch.randint(-1, 2, (len(counts), 2 * inter, k), generator=g).to(F64)
    xs = x[rt.gather.long()] if gathered else x
    ref = torch.empty(rt.slots, inter, dtype=F64)
    for e in range(len(counts)):
        a, b = rt.offsets[e].item(), rt.offsets[e + 1].item()
        s = xs[a:b] @ w[e].t()
        assert b == a or s.abs().max().item() <= SWIGLU_MAX_SUM
        gu = s * 2.0 ** -6
        ref[a:b] = gu[:, :inter] * torch.sigmoid(gu[:, :inter]) * gu[:, inter:]
    return MoeSwi(x.to(BF16), (w * 2.0 ** -6).to(BF16), ref)


@functools.lru_cache(maxsize=8)
def combine_case(t, top_k, h):
    """Integer ys [t top_k, h] (|y| <= 2000), power-of-two weights, an arbitrary inv permutation:
    every product has <= 11 + 3 significant bits and the sum of top_k of them is exact in f32."""
    g = gen(t, top_k, h, 13)
    ys = torch.randint(-2000, 2001, (t * top_k, h), generator=g).to(BF16)      # bf16-rounded integers
    topk_w = torch.pow(2.0, -torch.randint(0, 4, (t, top_k), generator=g).float())
    inv = torch.randperm(t * top_k, generator=g).int()
    exact = (topk_w.double().unsqueeze(-1) * ys.double()[inv.long()].reshape(t, top_k, h)).sum(1)
    return Combine(ys, topk_w, inv, exact)


@functools.lru_cache(maxsize=8)
def route_case(t, e, top_k=2):
    """bf16 logits [t, e] whose top-k is separated by wide margins: the chosen experts get 8, 7, ...
    (1 apart), every other expert at most 2 (so >= 4 below the last chosen one); expert ``idle`` is
    chosen by nobody.  rx [t, 64], rw [e, 64]: x and router weights whose product is exactly these
    logits (rw rows are unit vectors), for the fused router."""
    g = gen(t, e, top_k, 17)
    idle = (t + e) % e
    others = torch.tensor([i for i in range(e) if i != idle])
    logits = (torch.randint(-8, 9, (t, e), generator=g).float() * 0.25)        # [-2, 2], exact in bf16
    ids = others[torch.rand(t, e - 1, generator=g).argsort(1)[:, :top_k]]
    for j in range(top_k):
        logits[torch.arange(t), ids[:, j]] = 8.0 - j
    logits[:, idle] = -4.0
    h = 64
    rx = torch.zeros(t, h)
    rx[:, :e] = logits
    rx[:, e:] = torch.randint(-2, 3, (t, h - e), generator=g).float()          # multiplied by zeros
    rw = torch.zeros(e, h)
    rw[torch.arange(e), torch.arange(e)] = 1.0
    return RouteCase(logits.to(BF16), ids.int(), idle, rx.to(BF16), rw.to(BF16))
