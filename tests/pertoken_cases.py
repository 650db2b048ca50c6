"""Inputs, fp64 expectations and acceptance rules for the per-token kernels of
csrc/kernels/norm_elementwise.hip (rms_norm / rms_norm_q8, rope_cache_append + v_group_kernel,
silu_mul, embedding, add_inplace, argmax) and the fused decode append of attention.hip -- shared by
tests/test_pertoken_exact.py (GPU: the launches) and tests/test_pertoken_cases.py (CPU: the builders,
their preconditions and the proof that the rules reject wrong kernels).

Everything is built on the CPU from a seed derived from the shape (gemm_exact_cases.gen).  Random
operands are random bf16 BIT PATTERNS: sign and the 7 mantissa bits free, the exponent uniform in a
stated range, so outputs span many binades.

Acceptance rules
  exact      torch.equal on the int16 views against bf16(fp64 result): used where the builder has
             asserted that the f32 evaluation is exact in any order, with or without FMA, so the one
             rounding left is the bf16 store (which the comparison then pins to nearest-even)
  rel        |y - ref| <= (2^-8 + 2^-12) |ref| against fp64: half a bf16 ulp (2^-8 |ref| at the most)
             plus f32 slack, no absolute term (SWIGLU_ATOL = 1e-30 is added only where the
             output can be denormal: silu)
  rope real  |y - ref| <= 2^-8 |ref| + 2^-22 (|a c| + |b s|): a c - b s can cancel, so the f32
             evaluation error is absolute in the operands (two products and one sum, each within
             2^-24 of its own magnitude: <= 2^-23 (|a c| + |b s|), taken twice), plus half a bf16
             ulp of the result
"""
import functools
from collections import namedtuple

import torch

import gemm_exact_cases as gx
from gemm_exact_cases import BF16, F64, SENT16, gen

I16 = torch.int16
EPS = 1e-5
BF16_MAX = 3.3895313892515355e38


# ---------------------------------------------------------------- bit patterns and stores
def patterns(g, shape, emin, emax):
    """Random bf16 bit patterns: random sign, exponent uniform in 2^emin .. 2^emax, 7 random mantissa bits."""
    sign = torch.randint(0, 2, shape, generator=g)
    exp = torch.randint(127 + emin, 127 + emax + 1, shape, generator=g)
    man = torch.randint(0, 128, shape, generator=g)
    return from_bits((sign << 15) | (exp << 7) | man)


def from_bits(bits):
    """int64 values in [0, 65536) -> the bf16 tensor with those bit patterns."""
    return torch.where(bits >= 32768, bits - 65536, bits).to(I16).view(BF16)


def trunc_bf16(y32):
    """f32 -> bf16 by dropping the low 16 bits (the wrong store that the mutation checks emulate)."""
    return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def tie_share(s32):
    """Share of the f32 values that sit exactly half way between two bf16 values."""
    return ((s32.contiguous().view(torch.int32) & 0xFFFF) == 0x8000).double().mean().item()


def rounded_share(y64):
    return (y64.to(BF16).to(F64) != y64).double().mean().item()


def same_bits(y, expected):
    """None if the two bf16 tensors hold the same bits, else a message naming the first mismatch."""
    expected = expected.to(y.device)
    if y.shape == expected.shape and torch.equal(y.contiguous().view(I16), expected.contiguous().view(I16)):
        return None
    y2, e2 = y.reshape(-1, y.shape[-1]), expected.reshape(-1, expected.shape[-1])
    return gx.bits_mismatch(y2, e2) or "the values compare equal but their bits differ (sign of zero / NaN payload)"


def assert_same_bits(y, expected):
    msg = same_bits(y, expected)
    assert msg is None, msg


def rel_mismatch(y, ref, slack=None, rtol=gx.SWIGLU_RTOL, kinds=None):
    """None if |y - ref| <= rtol |ref| (+ slack) everywhere, else a message naming the worst element."""
    ref = ref.to(y.device)
    err = (y.to(F64) - ref).abs()
    bound = rtol * ref.abs()
    if slack is not None:
        bound = bound + slack.to(y.device)
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return None
    i = torch.argmax(torch.where(bad, err / bound.clamp(min=1e-300), torch.zeros_like(err))).item()
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), y.shape))
    kind = f" ({kinds[idx[0]]})" if kinds is not None else ""
    return (f"{int(bad.sum())} of {y.numel()} outside the bound; worst at {idx}{kind}: got {y[idx].item()!r}, "
            f"expected {ref[idx].item()!r}")


# ---------------------------------------------------------------- 1. RMSNorm
NORM_HIDDEN = [8, 136, 2048, 2056, 4096, 4104, 8192, 8200, 16384]
NormCase = namedtuple("NormCase", "x w ref kinds fx fres new_res fref fkinds hidden")


def norm_ref(r, w, eps=EPS):
    """fp64 r rsqrt(mean(r^2) + eps) w."""
    r, w = r.to(F64), w.to(F64)
    return r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w


def needle_columns(hidden):
    """The thread / wave / chunk boundaries of the reduction (vector v belongs to thread v % 256, chunk
    v / 256), clipped to the row, plus 7 seeded random columns."""
    fixed = [0, 7, 8 * 63 + 7, 8 * 64, 8 * 255 + 7, 8 * 256, hidden // 2, hidden - 8, hidden - 1]
    rnd = torch.randint(0, hidden, (7,), generator=gen(hidden, 501)).tolist()
    return sorted({min(c, hidden - 1) for c in fixed + rnd})


@functools.lru_cache(maxsize=None)
def norm_case(hidden):
    """x [rows, hidden] for the unfused form and (fx, fres) for the fused one, whose new residual
    new_res = bf16(fx + fres) is exact in f32 (asserted) and has the same kinds of rows:
      random  3 rows, x exponents 2^-8 .. 2^8
      needle  one row per needle column: background exponents 2^-7 .. 2^-5, one element +-64
              (fused: 96 - 32 and a second background of 2^-9 .. 2^-7)
      zero    all zero (fused: fres = -fx, an exact cancellation)
      tiny    |x| about 2^-20: eps dominates
      tie     (fused only) fres = +-2^-8 of fx's binade: fx + fres is half way between two bf16 values
    w: exponents 2^-4 .. 2^4."""
    g = gen(hidden, 500)
    cols = needle_columns(hidden)
    n = len(cols)
    w = patterns(g, (hidden,), -4, 4)
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(n)])
    ar = torch.arange(n)

    needle = patterns(g, (n, hidden), -7, -5)
    needle[ar, cols] = (64.0 * sign).to(BF16)
    x = torch.cat([patterns(g, (3, hidden), -8, 8), needle, torch.zeros(1, hidden, dtype=BF16),
                   patterns(g, (1, hidden), -21, -20)])
    kinds = ["random"] * 3 + [f"needle at {c}" for c in cols] + ["zero", "tiny"]

    fn_x, fn_r = patterns(g, (n, hidden), -7, -5), patterns(g, (n, hidden), -9, -7)
    fn_x[ar, cols] = (96.0 * sign).to(BF16)
    fn_r[ar, cols] = (-32.0 * sign).to(BF16)
    zx = patterns(g, (1, hidden), -8, 8)
    tx = patterns(g, (1, hidden), -2, 2)
    tbits = tx.view(I16).long() & 0xFFFF
    tr = from_bits((torch.randint(0, 2, (1, hidden), generator=g) << 15) | ((((tbits >> 7) & 0xFF) - 8) << 7))
    fx = torch.cat([patterns(g, (3, hidden), -8, 8), fn_x, zx, patterns(g, (1, hidden), -21, -20), tx])
    fres = torch.cat([patterns(g, (3, hidden), -8, 8), fn_r, -zx, patterns(g, (1, hidden), -22, -21), tr])
    fkinds = kinds + ["tie"]
    s32 = fx.float() + fres.float()
    assert torch.equal(s32.double(), fx.double() + fres.double()), "fx + fres must be exact in f32"
    new_res = s32.to(BF16)
    assert bool((new_res[3 + n] == 0).all()) and tie_share(s32[-1]) >= 0.4
    assert bool((new_res[3 + ar, cols].float() == 64.0 * sign).all())
    return NormCase(x, w, norm_ref(x, w), kinds, fx, fres, new_res, norm_ref(new_res, w), fkinds, hidden)


def norm_emulate(r, w, eps=EPS, drop_last_vector=False, no_eps=False, mean_over=None, truncate=False):
    """The kernel's formula in f32 torch: bf16(v * rsqrt(ss / hidden + eps) * w), and its wrong forms."""
    v = r.float()
    ss = (v[:, :-8] if drop_last_vector else v).pow(2).sum(-1, keepdim=True)
    inv = torch.rsqrt(ss / float(mean_over or r.shape[-1]) + (0.0 if no_eps else eps))
    y = v * inv * w.float()
    return trunc_bf16(y) if truncate else y.to(BF16)


# ---------------------------------------------------------------- 2. rope_cache_append
ROPE_SHAPES = [(32, 8, 128, 32), (12, 12, 64, 32), (4, 1, 128, 16), (8, 2, 64, 16), (2, 2, 256, 32), (3, 1, 8, 16)]
ROPE_TOKENS = [1, 7, 8, 9, 70]
ROPE_TABLES = ["dyadic", "none", "real", "llama3"]
MAX_POS = 512
ROPE_BLOCKS = 14
LLAMA3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
          "original_max_position_embeddings": 8192}
RopeCase = namedtuple("RopeCase", "qkv pos slots table q k v q64 k64 q_slack k_slack kidx vidx k_cache v_cache "
                                  "hq hkv d bs tokens")


def rope_slots(tokens, bs):
    """70 slots in the run pattern of test_rope_cache_append_prefill_groups, scaled to the block size.
    By groups of 8 tokens: 0-39 five aligned whole groups (every offset of a 32-key block, a block
    boundary between groups); 40-47 consecutive but starting mid-group; 48-55 an aligned group in
    descending order (non-consecutive); 56-63 consecutive, unaligned and across a block boundary;
    64-69 scattered singles, the ragged tail.  Fewer tokens take slots 24, 25, ...: 8 tokens are one
    aligned whole group at the end of a 32-key block, 9 add a tail token in the next block."""
    runs = [(0, 40), (3 * bs + 4, 8)]
    sl = [s + i for s, n in runs for i in range(n)] + [5 * bs + 7 - i for i in range(8)]
    sl += [6 * bs + 28 + i for i in range(8)] + [9 * bs + bs - 1, 10 * bs + 2, 11 * bs + 9, 12 * bs + 3, 12 * bs + 1,
                                                  13 * bs]
    assert len(sl) == 70
    return sl if tokens == 70 else sl[24:24 + tokens]


def rope_positions(tokens):
    """max_pos - 1 and 0, duplicates, a non-monotonic order."""
    base = [MAX_POS - 1, 0, 5, 5, 3, 200, 1, MAX_POS - 1, 0]
    rnd = torch.randint(0, MAX_POS, (70,), generator=gen(tokens, 502)).tolist()
    return (base + rnd)[:tokens]


@functools.lru_cache(maxsize=None)
def rope_table(kind, d):
    """[MAX_POS, d] f32, first half cos, second half sin; None for "none".
    dyadic: cos = +-2^e, sin = +-2^e', e = (5 pos + 3 p) mod 7 - 3, e' = (3 pos + 5 p + 1) mod 7 - 3 (5 and
    3 are units mod 7: rows and columns next to each other always differ), signs hashed from (pos, p)."""
    if kind == "none":
        return None
    if kind == "dyadic":
        pos, p = torch.arange(MAX_POS).view(-1, 1), torch.arange(d // 2).view(1, -1)
        e, e2 = (5 * pos + 3 * p) % 7 - 3, (3 * pos + 5 * p + 1) % 7 - 3
        sc = 1 - 2 * (((pos * 37 + p * 101 + (pos ^ p)) >> 2) & 1)
        ss = 1 - 2 * (((pos * 53 + p * 29 + (pos ^ (3 * p))) >> 1) & 1)
        return torch.cat([sc * torch.pow(2.0, e.double()), ss * torch.pow(2.0, e2.double())], dim=1).float()
    from distributed_llms_amd.ops import reference as ref
    return ref.rope_cos_sin(d, MAX_POS, 5e5, LLAMA3 if kind == "llama3" else None)


def rotate64(x, pos, table, pos_shift=0, pair_shift=0):
    """x [T, H, d] bf16 -> (rotated fp64 [T, H, d], |a c| + |b s| of every output).  ``pos_shift`` /
    ``pair_shift``: the wrong kernels that read row pos + 1 / the cos and sin of pair p + 1."""
    d = x.shape[-1]
    h = d // 2
    xf = x.to(F64)
    if table is None:
        return xf, torch.zeros_like(xf)
    cs = table.to(F64)[(torch.as_tensor(pos).long() + pos_shift) % table.shape[0]]
    pair = (torch.arange(h) + pair_shift) % h
    c, s = cs[:, :h][:, pair].unsqueeze(1), cs[:, h:][:, pair].unsqueeze(1)
    a, b = xf[..., :h], xf[..., h:]
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=-1)
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1), mag


def rotate32(x, pos, table, truncate=False, fma=False):
    """The kernels' f32 evaluation (plain, or attention.hip's fmaf(a, c, -(b s)) form through fp64,
    which holds the fused product exactly) with a nearest-even or a truncating store."""
    d = x.shape[-1]
    h = d // 2
    if table is None:
        return x.clone()
    cs = table[torch.as_tensor(pos).long()]
    c, s = cs[:, :h].unsqueeze(1), cs[:, h:].unsqueeze(1)
    a, b = x.float()[..., :h], x.float()[..., h:]
    if fma:
        o = torch.cat([(a.double() * c.double() - (b * s).double()).float(),
                       (b.double() * c.double() + (a * s).double()).float()], dim=-1)
    else:
        o = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    return trunc_bf16(o) if truncate else o.to(BF16)


def krow32(j):
    return ((j & 4) << 2) + ((j >> 3) << 2) + (j & 3)


def cache_indices(slots, hkv, d, bs, krow_identity=False, other_vofs=False):
    """(kidx, vidx) [T, hkv, d]: the flat element of k_cache [NB, hkv, bs, d] / v_cache [NB, hkv, d, bs]
    that holds (token, head, dim) -- common.h krow / vofs.  ``krow_identity`` / ``other_vofs``: the wrong
    layouts (a 32-key block with plain rows; the V^T order of the other block size)."""
    sl = torch.as_tensor(slots).long().view(-1, 1, 1)
    blk, off = sl // bs, sl % bs
    h, e = torch.arange(hkv).view(1, -1, 1), torch.arange(d).view(1, 1, -1)
    row = krow32(off) if bs == 32 and not krow_identity else off
    tiled = (off >> 3) * 8 * d + e * 8 + (off & 7)
    plain = e * bs + off
    vo = tiled if (bs == 32) != other_vofs else plain
    return ((blk * hkv + h) * bs + row) * d + e, (blk * hkv + h) * d * bs + vo


def fill_cache(shape, idx, values):
    """An int16 cache of sentinels with ``values`` (bf16) at the flat elements ``idx``."""
    c = torch.full(shape, SENT16, dtype=I16)
    c.view(-1)[idx.reshape(-1)] = values.contiguous().view(I16).reshape(-1)
    return c


@functools.lru_cache(maxsize=8)
def rope_case(hq, hkv, d, bs, tokens, kind):
    """qkv [T, (hq + 2 hkv) d]: exponents 2^-4 .. 2^4.  q / k: bf16 of the fp64 rotation, v a copy;
    k_cache / v_cache: the expected int16 caches, sentinels wherever no token writes.  With the dyadic
    table every product is exact and a c - b s needs at most 23 significand bits (8 + an exponent gap of
    at most 14 + a carry), so the f32 evaluation is exact in any order, with or without FMA -- asserted,
    with a rounded share of at least 50 %."""
    g = gen(hq, hkv, d, bs, tokens, 503)
    qkv = patterns(g, (tokens, (hq + 2 * hkv) * d), -4, 4)
    pos, slots = rope_positions(tokens), rope_slots(tokens, bs)
    assert all(0 <= p < MAX_POS for p in pos) and all(0 <= s < ROPE_BLOCKS * bs for s in slots)
    assert len(set(slots)) == tokens
    table = rope_table(kind, d)
    x = qkv.view(tokens, hq + 2 * hkv, d)
    xq, xk, v = x[:, :hq], x[:, hq:hq + hkv], x[:, hq + hkv:]
    q64, qmag = rotate64(xq, pos, table)
    k64, kmag = rotate64(xk, pos, table)
    if kind == "dyadic":
        for x_, y64 in ((xq, q64), (xk, k64)):
            assert torch.equal(rotate32(x_, pos, table), y64.to(BF16))
            assert torch.equal(rotate32(x_, pos, table, fma=True), y64.to(BF16))
            assert torch.equal(y64.float().double(), y64) and rounded_share(y64) >= 0.5
    kidx, vidx = cache_indices(slots, hkv, d, bs)
    k = k64.to(BF16)
    return RopeCase(qkv, torch.tensor(pos, dtype=torch.int32), torch.tensor(slots, dtype=torch.int32), table,
                    q64.to(BF16), k, v.contiguous(), q64, k64, 2.0 ** -22 * qmag, 2.0 ** -22 * kmag, kidx, vidx,
                    fill_cache((ROPE_BLOCKS, hkv, bs, d), kidx, k), fill_cache((ROPE_BLOCKS, hkv, d, bs), vidx, v),
                    hq, hkv, d, bs, tokens)


def rope_real_mismatch(y, ref64, slack):
    """The real-table rule: half a bf16 ulp of |ref| plus 2^-22 (|a c| + |b s|) of f32 evaluation error."""
    return rel_mismatch(y, ref64, slack=slack, rtol=2.0 ** -8)


# fused decode append (attention.hip, 32-key blocks): (hq, hkv, d) x lens
DECODE_SHAPES = [(32, 8, 128), (12, 12, 64)]
DECODE_LENS = [[1], [7, 33, 100]]
DecodeCase = namedtuple("DecodeCase", "qkv pos slots table k0 v0 k_cache v_cache q block_tables seq_lens")


@functools.lru_cache(maxsize=4)
def decode_rope_case(hq, hkv, d, lens):
    """One new token per sequence at position len - 1 with the dyadic table.  The k / v parts of qkv have
    exponents 2^-4 .. 2^4 (the exact case above); the q part 2^-8 .. 2^-4 and the cache's earlier contents
    2^-3 .. 2^0, which keeps the scores of the attention that follows moderate.  k_cache / v_cache: the
    previous contents (k0 / v0, every block, also those of no sequence) with the new key in place."""
    bs, b = 32, len(lens)
    g = gen(hq, hkv, d, sum(lens), b, 504)
    nblocks = [(n + bs - 1) // bs for n in lens]
    nb = sum(nblocks) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    bt = torch.zeros(b, max(nblocks), dtype=torch.int32)
    i = 0
    for s, n in enumerate(nblocks):
        bt[s, :n] = torch.tensor(perm[i:i + n])
        i += n
    slots = [int(bt[s, (n - 1) // bs]) * bs + (n - 1) % bs for s, n in enumerate(lens)]
    pos = [n - 1 for n in lens]
    assert all(0 <= p < MAX_POS for p in pos) and all(0 <= s < nb * bs for s in slots)
    qkv = torch.cat([patterns(g, (b, hq * d), -8, -4), patterns(g, (b, 2 * hkv * d), -4, 4)], dim=1)
    k0, v0 = patterns(g, (nb, hkv, bs, d), -3, 0), patterns(g, (nb, hkv, d, bs), -3, 0)
    table = rope_table("dyadic", d)
    x = qkv.view(b, hq + 2 * hkv, d)
    q64, _ = rotate64(x[:, :hq], pos, table)
    k64, _ = rotate64(x[:, hq:hq + hkv], pos, table)
    for x_, y64 in ((x[:, :hq], q64), (x[:, hq:hq + hkv], k64)):
        assert torch.equal(rotate32(x_, pos, table, fma=True), y64.to(BF16)) and torch.equal(y64.float().double(), y64)
    kidx, vidx = cache_indices(slots, hkv, d, bs)
    kc, vc = k0.clone(), v0.clone()
    kc.view(-1)[kidx.reshape(-1)] = k64.to(BF16).reshape(-1)
    vc.view(-1)[vidx.reshape(-1)] = x[:, hq + hkv:].reshape(-1)
    return DecodeCase(qkv, torch.tensor(pos, dtype=torch.int32), torch.tensor(slots, dtype=torch.int32), table, k0, v0,
                      kc, vc, q64.to(BF16), bt, torch.tensor(lens, dtype=torch.int32))


# ---------------------------------------------------------------- 3. silu_mul
SILU_UPS = [1.0, -1.0, 0.75, -1.5, 1.25, -0.5, 2.0 ** -7 * 1.171875, -3e-3]
SILU_PAIRS = 65536 * 8
SILU_SHAPES = [(65536, 8), (1024, 512), (255, 2056), (2049, 2048)]
SiluCase = namedtuple("SiluCase", "gu ref finite expected")


@functools.lru_cache(maxsize=1)
def silu_pairs():
    """Every bf16 gate bit pattern with each of the 8 up values: pair j has gate bits j mod 65536 and up
    SILU_UPS[j / 65536].  -> (gate, up, ref fp64 = g sigmoid(g) u, finite, expected bf16): ``finite`` marks
    the pairs whose ref is finite and below the bf16 maximum (the tolerance rule applies); everywhere
    else -- NaN gates, +-inf, -inf x 0, overflow -- ``expected`` = ref.to(bf16) is compared by bits."""
    j = torch.arange(SILU_PAIRS)
    gate = from_bits(j & 0xFFFF)
    up = torch.tensor(SILU_UPS, dtype=torch.float32).to(BF16)[j >> 16]
    g, u = gate.to(F64), up.to(F64)
    ref = g * torch.sigmoid(g) * u
    finite = torch.isfinite(ref) & (ref.abs() < BF16_MAX)
    return gate, up, ref, finite, ref.to(BF16)


@functools.lru_cache(maxsize=1)
def silu_case(t, inter):
    """gu [t, 2 inter] = [gate | up]: element (r, c) is pair (r inter + c) mod 524288."""
    gate, up, ref, finite, expected = silu_pairs()
    j = torch.arange(t * inter) % SILU_PAIRS
    gu = torch.cat([gate[j].view(t, inter), up[j].view(t, inter)], dim=1).contiguous()
    return SiluCase(gu, ref[j].view(t, inter), finite[j].view(t, inter), expected[j].view(t, inter))


def silu_mismatch(y, case):
    """The silu rule on an output [t, inter]: swiglu_mismatch (rtol 2^-8 + 2^-12, atol 1e-30) where the
    reference is finite, the bits of ref.to(bf16) elsewhere, NaN matching NaN."""
    fin, zero = case.finite.to(y.device), torch.zeros((), dtype=y.dtype, device=y.device)
    msg = gx.swiglu_mismatch(torch.where(fin, y, zero), torch.where(case.finite, case.ref, torch.zeros((), dtype=F64)))
    if msg is not None:
        return "finite pairs: " + msg
    msg = gx.bits_mismatch(torch.where(fin, zero, y), torch.where(case.finite, zero.cpu(), case.expected))
    return None if msg is None else "non-finite pairs: " + msg


def rn_share(y, case):
    """Share of the finite pairs whose output is the correctly rounded reference."""
    fin = case.finite.to(y.device)
    return ((y == case.expected.to(y.device)) & fin).sum().item() / fin.sum().item()


def silu_emulate(gu, truncate=False, clamp=None):
    """The kernel's formula in f32 torch: bf16(x / (1 + exp(-x)) * u).  ``clamp``: the wrong kernel that
    clamps the argument of exp to |x| <= clamp."""
    i = gu.shape[1] // 2
    x, u = gu[:, :i].float(), gu[:, i:].float()
    xe = x if clamp is None else torch.where(torch.isnan(x), x, x.clamp(-clamp, clamp))
    y = x * (1.0 / (1.0 + torch.exp(-xe))) * u
    return trunc_bf16(y) if truncate else y.to(BF16)


# ---------------------------------------------------------------- 4. embedding, add_, argmax
EMB_HIDDEN = [8, 512, 2048, 2056, 8192]
EMB_VOCAB = 300
EmbCase = namedtuple("EmbCase", "table ids expected")


@functools.lru_cache(maxsize=2)
def embedding_case(hidden):
    """Table element (r, c) holds the int16 pattern (8209 r + c) mod 2^16: 8209 is odd and hidden <= 2^16,
    so no two elements of a row and no two of a column are equal.  Ids: 0, vocab - 1, duplicates, random
    ids, and -1, -2^31, vocab, 2^31 - 1, which the kernel clamps to rows 0 and vocab - 1."""
    v = EMB_VOCAB
    r, c = torch.arange(v).view(-1, 1), torch.arange(hidden).view(1, -1)
    table = from_bits((8209 * r + c) & 0xFFFF)
    rnd = torch.randint(0, v, (9,), generator=gen(hidden, 505)).tolist()
    ids = [0, v - 1, 17, 17, 0] + rnd + [-1, -2 ** 31, v, 2 ** 31 - 1]
    rows = torch.tensor([min(max(i, 0), v - 1) for i in ids])
    return EmbCase(table, torch.tensor(ids, dtype=torch.int32), table[rows])


ADD_N = [8, 8 * 2049, 8 * (2048 * 256 + 1)]
AddCase = namedtuple("AddCase", "a b expected ties")


@functools.lru_cache(maxsize=1)
def add_case(n):
    """a, b [n / 8, 8]: exponents 2^-8 .. 2^8 (8 significand bits + a gap of at most 16: the f32 sum is
    exact, asserted); the first quarter has b = -a, the second b = +-2^-8 of a's binade (ties)."""
    g = gen(n, 506)
    a, b = patterns(g, (n,), -8, 8), patterns(g, (n,), -8, 8)
    q = max(1, n // 4)
    b[:q] = -a[:q]
    abits = a[q:2 * q].view(I16).long() & 0xFFFF
    b[q:2 * q] = from_bits((torch.randint(0, 2, (q,), generator=g) << 15) | ((((abits >> 7) & 0xFF) - 8) << 7))
    s32 = a.float() + b.float()
    assert torch.equal(s32.double(), a.double() + b.double()), "a + b must be exact in f32"
    return AddCase(a.view(-1, 8), b.view(-1, 8), s32.to(BF16).view(-1, 8), tie_share(s32))


ARGMAX_VOCAB = [50257, 1000, 7]
ARGMAX_PAD = [24, 3]
ARGMAX_ROWS = 5


@functools.lru_cache(maxsize=2)
def argmax_case(vocab, pad):
    """buf [rows, vocab + pad]: in-vocabulary exponents 2^-4 .. 2^4 (|x| < 32, many equal maxima), the
    padding columns 1000.  -> (buf, expected): the argmax of the [:, :vocab] view."""
    buf = patterns(gen(vocab, pad, 507), (ARGMAX_ROWS, vocab + pad), -4, 4)
    buf[:, vocab:] = 1000.0
    assert buf[:, :vocab].float().max() < 1000.0
    return buf, buf[:, :vocab].float().argmax(-1).to(torch.int32)
