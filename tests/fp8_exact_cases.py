"""FP8 (W8A8) operands whose GEMM / quantization result is known to the last bit, their fp64 and
emulated references and the preconditions that make the comparison exact -- shared by
tests/test_fp8_exact.py (GPU) and tests/test_fp8_cases.py (CPU: the builders, the preconditions and
the mutants of the emulation).  Derivations: test_fp8_exact.py's docstring.

Operands are built directly as e4m3 bytes (uint8, viewed as torch.float8_e4m3fn by the GPU tests)
with hand-chosen f32 scale vectors, on the CPU, from a seed derived from the shape."""
import functools
from collections import namedtuple

import numpy as np
import torch

from gemm_exact_cases import (BF16, F64, GUARD_M, MIN_ROUNDED, MIN_TIES, SLAB_LIMIT, SWIGLU_MAX_SUM, WIDE_M, bf16_shares,
                              gen, slice_rule, survives_slab)
from moe_exact_cases import ROUTINGS, routing

E4M3 = torch.float8_e4m3fn
F32 = torch.float32
U8 = torch.uint8
ONE = 0x38                        # e4m3 1.0
NAN_BYTE = 0x7F                   # e4m3 NaN: the fill of the guard rows around xq and wq
KT = 128                          # an FP8 K-tile

Fp8Int = namedtuple("Fp8Int", "xq wq sa sb acc expected rounded ties m n k r")
Fp8Sel = namedtuple("Fp8Sel", "xq wq sa sb expected rows")
Fp8Swi = namedtuple("Fp8Swi", "xq wq sa sb ref gmax")
Fp8Moe = namedtuple("Fp8Moe", "xq wq sa wscale acc expected ref")
QuantRows = namedtuple("QuantRows", "x q scale ties")


def decode(q):
    """e4m3 bytes -> fp64 values."""
    return q.view(E4M3).to(F64)


def encode(v):
    """fp64 values that e4m3 holds exactly -> bytes (asserted)."""
    q = v.to(F32).to(E4M3)
    assert torch.equal(q.to(F64), v.to(F64)), "not exact in e4m3"
    return q.view(U8)


def fp8_slices(k, splits):
    """(S, [(a, b), ...]): gemm_wide_fp8's K slices -- slice_rule on k // 2, an FP8 K-tile being 128
    wide (the bytes of a 64-K bf16 tile)."""
    s, kts = slice_rule(k // 2, splits)
    return s, [(i * kts * KT, min(k, (i + 1) * kts * KT)) for i in range(s)]


def through_slab(v):
    """f32 values through the split-K slab format: f16(v 2^-6) 64."""
    return (v.to(F32) * 2.0 ** -6).half().float() * 64.0


def pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=F64), e.to(F64)).to(F32)


# ------------------------------------------------------------------ integer operands
def int_scales(m, n):
    """sa[m] = 2^((m mod 5) - 2), sb[n] = 2^((n mod 7) - 3): distinct along both axes, so a scale
    read one row or column off changes the result by a factor of two or more."""
    return pow2(torch.arange(m) % 5 - 2), pow2(torch.arange(n) % 7 - 3)


def general_scales(m, n, seed=0):
    """Random f32 in [2^-6, 2^2] with full mantissas."""
    g = gen(m, n, seed, 41)
    sa = torch.pow(2.0, torch.rand(m, generator=g, dtype=F64) * 8 - 6).to(F32)
    sb = torch.pow(2.0, torch.rand(n, generator=g, dtype=F64) * 8 - 6).to(F32)
    assert bool(((sa.view(torch.int32) & 0xFFFF) != 0).float().mean() > 0.9)
    return sa, sb


def epilogue_f32(acc, sa, sb):
    """The epilogue's arithmetic, v * (sa[m] * sb[n]): two f32 multiplies, no addition (nothing to
    contract into an FMA), emulated in numpy float32."""
    s = sa.numpy().astype(np.float32)[:, None] * sb.numpy().astype(np.float32)[None, :]
    a32 = acc.numpy().astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc.numpy())
    return torch.from_numpy((a32 * s).astype(np.float32))


@functools.lru_cache(maxsize=12)
def int_case(m, n, k, r=8, scales="pow2", seed=0):
    """xq [m, k], wq [n, k]: uniform integers in [-r, r], r <= 8, all exact in e4m3 (4 significant
    bits hold 0 .. 16).  Every partial sum is an integer of magnitude <= r^2 K <= 64 K < 2^24: exact
    in f32 in any order.  scales "pow2": expected = bf16(acc sa sb) from fp64, with the rounded / tie
    shares asserted on acc (powers of two do not move ties); "general": expected =
    bf16(f32(f32(acc) f32(sa sb))), unsplit launches only."""
    assert r <= 8 and r * r * k < 2 ** 24, (k, r)
    g = gen(m, n, k, r, seed, 8)
    x = torch.randint(-r, r + 1, (m, k), generator=g).to(F64)
    w = torch.randint(-r, r + 1, (n, k), generator=g).to(F64)
    acc = x @ w.t()
    assert acc.abs().max().item() < 2 ** 24
    rounded, ties = bf16_shares(acc)
    if scales == "pow2":
        sa, sb = int_scales(m, n)
        assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, (m, n, k, r, rounded, ties)
        exact = acc * sa.to(F64)[:, None] * sb.to(F64)[None, :]
        assert torch.equal(epilogue_f32(acc, sa, sb).to(F64), exact)      # exact in f32 as well
        expected = exact.to(BF16)
    else:
        sa, sb = general_scales(m, n, seed)
        expected = epilogue_f32(acc, sa, sb).to(BF16)
    return Fp8Int(encode(x), encode(w), sa, sb, acc, expected, rounded, ties, m, n, k, r)


def check_slabs(case, splits):
    """Precondition of every split launch: each slice's scaled partial passes through the f16 x 2^-6
    slab unchanged.  |partial| <= 2048 gives the 11 bits; the scale product 2^-5 .. 2^4 keeps
    |partial| 2^-6 sa sb inside f16's normal range (>= 2^-11, <= 2^9).  -> the largest |partial|."""
    return check_slabs_of(case.xq, case.wq, case.sa, case.sb, splits)


def check_slabs_of(xq, wq, sa, sb, splits):
    k = xq.shape[1]
    s, slices = fp8_slices(k, splits)
    if s == 1:
        return 0.0
    x, w = decode(xq), decode(wq)
    worst = 0.0
    for a, b in slices:
        p = x[:, a:b] @ w[:, a:b].t()
        worst = max(worst, p.abs().max().item())
        v = epilogue_f32(p, sa, sb)
        assert torch.equal(through_slab(v), v), (tuple(xq.shape), tuple(wq.shape), splits, "scaled partial changed by the slab")
    assert worst <= SLAB_LIMIT, (tuple(xq.shape), tuple(wq.shape), splits, worst)
    return worst


# ------------------------------------------------------------------ selector
FINITE_CODES = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF, 0x80)], dtype=torch.int64)


@functools.lru_cache(maxsize=8)
def selector_case(m, n, k, seed=0):
    """xq: a row-permuted identity (m >= k, one 1.0 per used row); wq: random e4m3 bit patterns over
    every code but NaN (0x7F, 0xFF) and -0 (0x80: 0 + -0 = +0), subnormals included; unit scales.
    y[rows[j], :] == bf16(wq[:, j]) bit for bit and every other row is 0.  Every finite e4m3 value
    is exact in bf16 and, after 2^-6, in f16 (asserted), so split launches are covered."""
    assert m >= k
    g = gen(m, n, k, seed, 78)
    rows = torch.randperm(m, generator=g)[:k]
    xq = torch.zeros(m, k, dtype=U8)
    xq[rows, torch.arange(k)] = ONE
    wq = FINITE_CODES[torch.randint(0, FINITE_CODES.numel(), (n, k), generator=g)].to(U8)
    w = decode(wq)
    assert bool(torch.isfinite(w).all())
    assert torch.equal(w.to(BF16).to(F64), w) and bool(survives_slab(w.to(BF16)).all())
    assert bool((w.abs() < 2.0 ** -6).any()) and bool((w.abs() == 448).any())      # subnormals and the maximum
    expected = torch.zeros(m, n, dtype=BF16)
    expected[rows] = w.t().contiguous().to(BF16)
    return Fp8Sel(xq, wq, torch.ones(m), torch.ones(n), expected, rows)


# ------------------------------------------------------------------ ternary SwiGLU
@functools.lru_cache(maxsize=8)
def swiglu_case(m, inter, k, seed=0):
    """xq in {-1, 0, 1}, wq = [Wg; Wu] [2 inter, k] in {-1, 0, 1}, sb = 2^-6, sa = 1.  Every gate / up
    sum is an integer of magnitude <= 256 (asserted): exact in f32 and, times 2^-6, in the slabs.
    ref = silu(g) u in fp64."""
    g = gen(m, inter, k, seed, 34)
    x = torch.randint(-1, 2, (m, k), generator=g).to(F64)
    w = torch.randint(-1, 2, (2 * inter, k), generator=g).to(F64)
    sums = x @ w.t()
    gmax = sums.abs().max().item()
    assert gmax <= SWIGLU_MAX_SUM, (m, inter, k, gmax)
    gu = sums * 2.0 ** -6
    assert torch.equal(through_slab(gu.float()).to(F64), gu)
    gate, up = gu[:, :inter], gu[:, inter:]
    return Fp8Swi(encode(x), encode(w), torch.ones(m), torch.full((2 * inter,), 2.0 ** -6), gate * torch.sigmoid(gate) * up,
                  gmax)


# ------------------------------------------------------------------ grouped (MoE) kernel
MOE_ROUTINGS = list(ROUTINGS) + [((0, 1, 64, 65, 128, 129, 200, 7), 2)]      # crosses the 64 / 128-row tile choice
# (n, k) of mode 0 and (inter, k) of mode 1 by [gathered]: the INT_DIMS / SWIGLU_DIMS pairs of
# moe_exact_cases whose K is a multiple of 128 (all of them are)
MOE_INT_DIMS = {True: (512, 256), False: (256, 512)}
MOE_SWIGLU_DIMS = {True: (256, 256), False: (128, 512)}


@functools.lru_cache(maxsize=8)
def moe_case(counts, top_k, n, k, gathered, mode):
    """mode 0: integer xq ([T, k] when gathered, else [slots, k]) and per-expert integer wq [E, n, k];
    sa[slot] = 2^((slot mod 5) - 2) in slot order, wscale[e, c] = 2^(((3 e + c) mod 7) - 3);
    expected[slot] = bf16(acc sa wscale).  mode 1 (n = 2 inter): ternary operands, sa[slot] =
    2^-(slot mod 3), wscale[e, c] = 2^(-6 - ((e + c) mod 4)), so |gate|, |up| <= 4; ref = silu(g) u."""
    rt = routing(counts, top_k)
    e = len(counts)
    r = 8 if mode == 0 else 1
    g = gen(rt.slots, n, k, int(gathered), mode, 19)
    x = torch.randint(-r, r + 1, (rt.t if gathered else rt.slots, k), generator=g).to(F64)
    w = torch.randint(-r, r + 1, (e, n, k), generator=g).to(F64)
    xs = x[rt.gather.long()] if gathered else x
    acc = torch.empty(rt.slots, n, dtype=F64)
    for j in range(e):
        a, b = rt.offsets[j].item(), rt.offsets[j + 1].item()
        acc[a:b] = xs[a:b] @ w[j].t()
    slot = torch.arange(rt.slots)
    ch = torch.arange(n)[None, :] + torch.arange(e)[:, None] * (3 if mode == 0 else 1)
    if mode == 0:
        sa, wscale = pow2(slot % 5 - 2), pow2(ch % 7 - 3)
        rounded, ties = bf16_shares(acc)
        assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, (rounded, ties)
    else:
        sa, wscale = pow2(-(slot % 3)), pow2(-6 - ch % 4)
        assert acc.abs().max().item() <= SWIGLU_MAX_SUM
    if gathered:                                           # by-token scales must differ from by-slot ones
        assert bool((sa[rt.gather.long()] != sa).any())
    scaled = acc * sa.to(F64)[:, None] * wscale.to(F64)[rt.slot_expert.long()]
    expected = ref = None
    if mode == 0:
        expected = scaled.to(BF16)
    else:
        gate, up = scaled[:, :n // 2], scaled[:, n // 2:]
        assert gate.abs().max().item() <= 4
        ref = gate * torch.sigmoid(gate) * up
    return Fp8Moe(encode(x), encode(w), sa, wscale, acc, expected, ref)


# ------------------------------------------------------------------ quantize_rows at its edges
def e4m3_grid():
    """Every non-negative finite e4m3 value, ascending (127 of them: 0, 2^-9, ..., 448)."""
    v = decode(torch.arange(0, 0x7F, dtype=torch.int64).to(U8))
    assert bool((v[1:] > v[:-1]).all()) and v[-1].item() == 448 and v[1].item() == 2.0 ** -9
    return v


def quantize_emulated(x, rounding="rne", nan="propagate"):
    """Per-row absmax e4m3 quantization of bf16 rows from first principles, in fp64: scale = amax /
    448 (f32 division; 1 for a zero row; non-finite for a row with a NaN or an Inf), q =
    round(clamp(x / scale)) on the e4m3 grid (step 2^(max(e, -6) - 3)).  Mutants: rounding "trunc"
    (toward zero), nan "clamp" (fmaxf-style: NaN never reaches amax and converts as -448)."""
    xf = x.to(F32)
    if nan == "clamp":
        amax = torch.nan_to_num(xf.abs(), nan=0.0, posinf=float("inf")).amax(dim=1)
    else:
        amax = xf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    v = (xf / scale[:, None]).to(F64)
    if nan == "clamp":
        v = torch.nan_to_num(v, nan=-448.0)
    v = v.clamp(-448, 448)
    a = v.abs()
    e = torch.floor(torch.log2(a.clamp(min=2.0 ** -20))).clamp(min=-6)
    step = torch.pow(torch.tensor(2.0, dtype=F64), e - 3)
    nsteps = a / step
    nsteps = torch.floor(nsteps) if rounding == "trunc" else torch.from_numpy(np.rint(nsteps.numpy()))
    out = torch.copysign(nsteps * step, v)
    return out.to(F32).to(E4M3).view(U8), scale


@functools.lru_cache(maxsize=24)
def quant_rows_case(m, k, seed=0):
    """bf16 rows for quant_fp8_rows: row i holds 448 c_i once (c_i a power of two, so scale[i] = c_i
    exactly and x / scale is exact) and c_i times values at the edges of the e4m3 conversion: every
    midpoint between two neighbouring e4m3 values (5 significant bits: exact in bf16; 2^-10 and
    3 2^-10 are the subnormal ones), 2^-11 (below half the smallest subnormal), +-0, 446 (the last
    bf16 value below 448; 447 and 449 do not exist in bf16, and a value above 448 would be the row's
    amax) and some grid values.  Asserted: >= 5 % of the elements are exact ties and the reference
    quantizer sends each to the neighbour with an even code."""
    from distributed_llms_amd.ops import quant
    grid = e4m3_grid()
    mids = (grid[1:] + grid[:-1]) / 2
    even = torch.where(torch.arange(126) % 2 == 0, grid[:-1], grid[1:])          # code i or i + 1, the even one
    first = torch.tensor([17.0, 2.0 ** -10, 3 * 2.0 ** -10, -0.0, 446.0, 2.0 ** -11, 0.0], dtype=F64)
    pool = torch.cat([mids, -mids, torch.tensor([2.0 ** -9, 2.0 ** -11, -2.0 ** -11, 0.0, -0.0, 446.0, -446.0], dtype=F64),
                      grid[1::9], -grid[2::9]])
    g = gen(m, k, seed, 55)
    v = pool[torch.randint(0, pool.numel(), (m, k), generator=g)]
    v[:, :min(7, k - 1)] = first[:min(7, k - 1)]
    peak = torch.randint(min(7, k - 1), k, (m,), generator=g)
    sign = torch.randint(0, 2, (m,), generator=g).to(F64) * 2 - 1
    v[torch.arange(m), peak] = 448.0 * sign
    c = pow2((torch.arange(m) + seed) % 7 - 3)
    x64 = v * c.to(F64)[:, None]
    x = x64.to(BF16)
    assert torch.equal(x.to(F64), x64)
    a = v.abs()
    idx = torch.searchsorted(mids, a.reshape(-1).contiguous()).clamp(max=125).reshape(a.shape)
    is_tie = mids[idx] == a
    ties = is_tie.double().mean().item()
    assert ties >= 0.05, (m, k, ties)
    q, s = quant.quantize_rows_ref(x)
    assert torch.equal(s, c), "scale[i] must be c_i exactly"
    assert torch.equal(decode(q.view(U8)).abs()[is_tie], even[idx][is_tie]), "reference must round ties to even"
    qe, se = quantize_emulated(x)
    assert torch.equal(qe, q.view(U8)) and torch.equal(se, s)
    return QuantRows(x, q.view(U8), s, ties)


QUANT_K = [8, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392]      # the MAXV dispatch edges; 16392 re-reads


E2e = namedtuple("E2e", "x w xq c wq d acc expected r")


@functools.lru_cache(maxsize=8)
def e2e_case(m, n, k, r=8, seed=0):
    """bf16 x [m, k] = c_m times integers in [-r, r] with x[:, 0] = +-448 c_m (c_m = 2^j), and w
    [n, k] likewise with d_n and w[:, 1] = +-448 d_n; x[:, 1] = w[:, 0] = 0, so the peaks -- which
    fix every scale at exactly c_m / d_n and every code at an integer -- add nothing to the product
    and a K slice's partial stays an integer within the slab's 11 bits.  quantize_rows /
    quantize_weight must return exactly xq, c / wq, d, and linear_fp8 then bf16(x w^T) from fp64."""
    g = gen(m, n, k, r, seed, 61)

    def side(rows, peak, hole, mod, lo):
        v = torch.randint(-r, r + 1, (rows, k), generator=g).to(F64)
        v[:, peak] = 448.0 * (torch.randint(0, 2, (rows,), generator=g).to(F64) * 2 - 1)
        v[:, hole] = 0
        c = pow2(torch.arange(rows) % mod + lo)
        return v, c, v * c.to(F64)[:, None]
    xv, c, x64 = side(m, 0, 1, 5, -2)
    wv, d, w64 = side(n, 1, 0, 7, -9)
    x, w = x64.to(BF16), w64.to(BF16)
    assert torch.equal(x.to(F64), x64) and torch.equal(w.to(F64), w64)
    acc = xv @ wv.t()
    assert acc.abs().max().item() <= r * r * k < 2 ** 24
    rounded, ties = bf16_shares(acc)
    assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, (m, n, k, r, rounded, ties)
    expected = (acc * c.to(F64)[:, None] * d.to(F64)[None, :]).to(BF16)
    return E2e(x, w, encode(xv), c, encode(wv), d, acc, expected, r)


# ------------------------------------------------------------------ emulation of the kernels' contract
def bf16_store(v, rounding="rne"):
    """f32 -> bf16: round to nearest even, or the truncating mutant."""
    v = v.to(F32)
    if rounding == "rne":
        return v.to(BF16)
    return (v.view(torch.int32) & -65536).view(F32).to(BF16)


def swap_chunks(t):
    """Mutant of ktile8's k map: the 16-byte chunks 2fq and 2fq + 1 of every 32-k group swapped."""
    k = t.shape[1]
    return t[:, torch.arange(k) ^ 16]


def emulate(xq, wq, sa, sb, splits=1, mutant=None):
    """The contract of gemm_wide_fp8, mode 0: per K slice the dequantized product in fp64 (exact),
    taken to f32, times f32(sa[m] sb[n]); with a K split through the f16 x 2^-6 slabs and summed in
    f32; stored as bf16 (RNE).  ``mutant``: one of the errors the cases exist to catch."""
    x, w = decode(xq), decode(wq)
    k = x.shape[1]
    if mutant == "sa_shift":
        sa = torch.roll(sa, 1)
    if mutant == "sb_shift":
        sb = torch.roll(sb, 1)
    if mutant == "swap_chunks":
        x = swap_chunks(x)
    s, slices = fp8_slices(k, splits)
    total = torch.zeros(x.shape[0], w.shape[0], dtype=F32)
    for a, b in slices:
        if mutant == "drop_tile" and s > 1:
            b -= KT
        v = epilogue_f32(x[:, a:b] @ w[:, a:b].t(), sa, sb)
        total = total + (through_slab(v) if s > 1 else v)
    return bf16_store(total, "trunc" if mutant == "trunc_store" else "rne")


def emulate_moe(case, rt, gathered, mutant=None):
    """The contract of moe_wide_gemm_fp8, mode 0; mutant "sa_by_token": sa read through gather."""
    x, w = decode(case.xq), decode(case.wq)
    xs = x[rt.gather.long()] if gathered else x
    sa = case.sa[rt.gather.long()] if mutant == "sa_by_token" else case.sa
    out = torch.empty(rt.slots, w.shape[1], dtype=BF16)
    for j in range(w.shape[0]):
        a, b = rt.offsets[j].item(), rt.offsets[j + 1].item()
        if b > a:
            out[a:b] = bf16_store(epilogue_f32(xs[a:b] @ w[j].t(), sa[a:b], case.wscale[j]))
    return out


def nonfinite_contract(scale, q, scale_clean, q_clean, j, kind):
    """None if (scale, q) of a run with a NaN / Inf (``kind``) in row j keeps the contract against
    the clean run, else what is wrong: scale[j] is NaN for a NaN, Inf or NaN for an Inf; every other
    row's q and scale are bit-identical."""
    sj = scale[j].item()
    if kind == "nan" and sj == sj:
        return f"scale[{j}] = {sj!r} for a row with a NaN"
    if kind == "inf" and not (sj != sj or abs(sj) == float("inf")):
        return f"scale[{j}] = {sj!r} for a row with an Inf"
    keep = torch.arange(scale.shape[0], device=scale.device) != j
    if not torch.equal(scale[keep].view(torch.int32), scale_clean[keep].view(torch.int32)):
        return "the scale of another row changed"
    if not torch.equal(q.view(U8)[keep], q_clean.view(U8)[keep]):
        return "the q of another row changed"
    return None


def poison(x, j, col, kind):
    xp = x.clone()
    xp[j, col] = float("nan") if kind == "nan" else float("inf") * (-1 if col % 2 else 1)
    return xp


# ------------------------------------------------------------------ case lists of the GPU tests
# integer GEMM: (m, n, k, r, splits, variant)
ROW_TILE_CASES = [(m, 256, 512, 8, s, 1) for m in WIDE_M for s in (1, 3)] + \
                 [(m, 256, 512, 8, s, 1 | (bm << 8)) for bm in (64, 128, 192, 256) for m in (65, 300) for s in (1, 3)]
VARIANT_CASES = [(129, 256, 1024, 4, s, v) for v in (1, 4) for s in (1, 3)] + \
                [(2100, 256, 256, 8, 1, 4 | 64), (2309, 384, 256, 8, 1, 4 | 64)]
SPLIT_CASES = [(65, 128, 128, 8, 1, 1), (65, 128, 384, 8, 2, 1), (65, 128, 1024, 8, 8, 1), (65, 128, 1024, 8, 16, 1),
               (64, 128, 14336, 2, 7, 1)]
GENERAL_CASES = [(m, 384, 256) for m in (1, 129, 300)]
GUARD_SHAPE = (256, 384, 8, 2)                      # n, k, r, splits: 3 K-tiles in slices of 2 and 1
SELECTOR_CASES = [(k, s, v) for k in (256, 512) for s, v in ((1, 1), (2, 1), (1, 1 | (64 << 8)), (2, 1 | (128 << 8)),
                                                             (1, 4 | (256 << 8)))]
SWIGLU_CASES = [(m, i, 256, s, 1) for m in (1, 65, 129, 300) for i in (64, 192) for s in (1, 2)] + \
               [(2100, 128, 256, 1, 4 | 64)]
# (m, n, k, r): M = 200 at K = 2048 takes the fp8_bm128 plan, (4 slices, 128-row tiles); (200, 256, 512) does not split
E2E_CASES = [(5, 256, 512, 8), (200, 256, 2048, 4), (300, 256, 512, 8)]


def all_int_cases():
    """Every (m, n, k, r, splits) of the pow2-scaled integer form that a GPU test launches."""
    out = [c[:5] for c in ROW_TILE_CASES + VARIANT_CASES + SPLIT_CASES]
    n, k, r, s = GUARD_SHAPE
    out += [(m, n, k, r, s) for m in GUARD_M] + [(65, 256, 512, 8, 1), (65, 256, 512, 8, 2)]
    return sorted(set(out))
