"""Inputs whose GEMM result is known to the last bit, their fp64 references and the preconditions
that make the comparison exact -- shared by tests/test_gemm_exact.py, tests/test_moe_exact.py (GPU)
and tests/test_exact_cases.py (CPU: the builders and preconditions themselves).

Everything is built on the CPU from a seed derived from the shape, so a case is the same tensors
wherever it is built; the derivations of the bounds are in test_gemm_exact.py's docstring."""
import functools
from collections import namedtuple

import torch

BF16 = torch.bfloat16
F64 = torch.float64
SLAB_LIMIT = 2048                 # |integer| <= 2^11 is exact as f16 x 2^-6 (11-bit significand)
MIN_ROUNDED, MIN_TIES = 0.05, 0.01
SWIGLU_RTOL = 2.0 ** -8 + 2.0 ** -12
SWIGLU_ATOL = 1e-30
SWIGLU_MAX_SUM = 256              # integers up to 2^8 are exact in bf16, and x 2^-12 in f16

IntCase = namedtuple("IntCase", "x w expected rounded ties m n k r")
SelCase = namedtuple("SelCase", "x w expected rows")
SwiCase = namedtuple("SwiCase", "x w ref gmax")


def gen(*key):
    """A CPU generator seeded from the integers ``key`` (a case's shape and a tag)."""
    g = torch.Generator()
    s = 0x9E3779B1
    for v in key:
        s = (s * 1000003 + int(v) + 12345) % (2 ** 62)
    g.manual_seed(s)
    return g


def slice_rule(k, splits):
    """(S, kts): the launchers' K-slice rule -- kts = ceil(K / 64 / splits) tiles per slice,
    S = ceil(K / 64 / kts) slices actually run."""
    kt = k // 64
    kts = -(-kt // splits)
    return -(-kt // kts), kts


def bf16_shares(y):
    """(rounded, ties): the share of the integer outputs ``y`` (fp64) that bf16 cannot hold, and the
    share that sits exactly half way between two bf16 values."""
    a = y.abs()
    e = torch.floor(torch.log2(a.clamp(min=1.0)))
    ulp = torch.pow(torch.tensor(2.0, dtype=F64), e - 7)
    rem = torch.where(ulp >= 2, torch.remainder(a, ulp.clamp(min=1.0)), torch.zeros_like(a))
    rounded = (y.to(BF16).to(F64) != y).double().mean().item()
    ties = ((ulp >= 2) & (rem * 2 == ulp)).double().mean().item()
    return rounded, ties


@functools.lru_cache(maxsize=12)
def int_case(m, n, k, r, seed=0):
    """x [m, k], w [n, k]: uniform integers in [-r, r] as bf16; expected = bf16(x @ w^T in fp64).
    Preconditions asserted here: K r^2 < 2^24 (every partial sum exact in f32, in any order), and
    the rounded / tie shares of the outputs (the comparison then also pins the rounding mode)."""
    assert r <= 256 and k * r * r < 2 ** 24, (k, r)
    g = gen(m, n, k, r, seed)
    x = torch.randint(-r, r + 1, (m, k), generator=g).to(F64)
    w = torch.randint(-r, r + 1, (n, k), generator=g).to(F64)
    y = x @ w.t()
    assert y.abs().max().item() < 2 ** 24
    rounded, ties = bf16_shares(y)
    assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, (m, n, k, r, rounded, ties)
    return IntCase(x.to(BF16), w.to(BF16), y.to(BF16), rounded, ties, m, n, k, r)


def max_slice_partial(case, splits):
    """Largest |partial sum| any of the S K-slices leaves in a slab (0 without a split)."""
    s, kts = slice_rule(case.k, splits)
    if s == 1:
        return 0.0
    x, w = case.x.to(F64), case.w.to(F64)
    worst = 0.0
    for i in range(s):
        a, b = i * kts * 64, min(case.k, (i + 1) * kts * 64)
        worst = max(worst, (x[:, a:b] @ w[:, a:b].t()).abs().max().item())
    return worst


def check_slabs(case, splits):
    """Precondition of every split launch: each slice's integer partial is exact in a slab."""
    worst = max_slice_partial(case, splits)
    assert worst <= SLAB_LIMIT, (case.m, case.n, case.k, case.r, splits, worst)
    return worst


def survives_slab(w):
    """True where a bf16 value passes through the f16 x 2^-6 slab format unchanged."""
    return (w.float() * 2.0 ** -6).half().float() * 64.0 == w.float()


@functools.lru_cache(maxsize=8)
def selector_case(m, n, k, seed=0):
    """x: k rows of an [m, k] zero matrix (a random choice, m >= k) hold one 1 each, at a different
    column each -- a row-permuted identity; w [n, k]: random bf16 bit patterns, both signs, exponents
    2^-8 .. 2^8, all 7 mantissa bits.  Then y[rows[j], :] == w[:, j] bit for bit and the other rows
    are 0."""
    assert m >= k
    g = gen(m, n, k, seed, 77)
    rows = torch.randperm(m, generator=g)[:k]
    x = torch.zeros(m, k, dtype=BF16)
    x[rows, torch.arange(k)] = 1.0
    sign = torch.randint(0, 2, (n, k), generator=g)
    exp = torch.randint(127 - 8, 127 + 9, (n, k), generator=g)
    man = torch.randint(0, 128, (n, k), generator=g)
    bits = (sign << 15) | (exp << 7) | man
    w = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(BF16)
    assert bool(torch.isfinite(w.float()).all()) and bool((w.float().abs() >= 2.0 ** -8).all())
    assert bool(survives_slab(w).all())
    expected = torch.zeros(m, n, dtype=BF16)
    expected[rows] = w.t().contiguous()
    return SelCase(x, w, expected, rows)


@functools.lru_cache(maxsize=8)
def swiglu_case(m, inter, k, seed=0):
    """x [m, k] in {-1, 0, 1}, w = [Wg; Wu] [2 inter, k] in {-1, 0, 1} x 2^-6.  Precondition: every
    gate / up sum is an integer of magnitude <= 256 before the scale, so gate and up are exact in
    f32, in bf16 and in the f16 slabs alike.  ref = silu(g) u in fp64."""
    g = gen(m, inter, k, seed, 33)
    x = torch.randint(-1, 2, (m, k), generator=g).to(F64)
    w = torch.randint(-1, 2, (2 * inter, k), generator=g).to(F64)
    sums = x @ w.t()
    gmax = sums.abs().max().item()
    assert gmax <= SWIGLU_MAX_SUM, (m, inter, k, gmax)
    gu = sums * 2.0 ** -6
    gate, up = gu[:, :inter], gu[:, inter:]
    ref = gate * torch.sigmoid(gate) * up
    return SwiCase(x.to(BF16), (w * 2.0 ** -6).to(BF16), ref, gmax)


def swiglu_mismatch(y, ref):
    """None if |y - ref| <= rtol |ref| + atol everywhere, else a message naming the worst element."""
    err = (y.to(F64) - ref.to(y.device)).abs()
    bound = SWIGLU_RTOL * ref.to(y.device).abs() + SWIGLU_ATOL
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return None
    i = torch.argmax(torch.where(bad, err / bound.clamp(min=1e-300), torch.zeros_like(err))).item()
    r, c = divmod(i, y.shape[1])
    return (f"{int(bad.sum())} of {y.numel()} outside rtol 2^-8 + 2^-12; worst at ({r}, {c}): got "
            f"{y[r, c].item()!r}, expected {ref[r, c].item()!r}")


def bits_mismatch(y, expected):
    """None if torch.equal(y, expected), else: count of mismatches, the first (m, n) and both values."""
    expected = expected.to(y.device)
    if y.shape == expected.shape and torch.equal(y, expected):
        return None
    if y.shape != expected.shape:
        return f"shape {tuple(y.shape)} vs {tuple(expected.shape)}"
    ne = ~((y == expected) | (torch.isnan(y) & torch.isnan(expected)))
    idx = ne.reshape(-1).nonzero()
    if idx.numel() == 0:                                  # they differ only where both are NaN
        return None
    i = idx[0].item()
    r, c = divmod(i, y.shape[-1])
    return (f"{idx.numel()} of {y.numel()} outputs differ; first at (m={r}, n={c}): got "
            f"{y.reshape(-1)[i].item()!r}, expected {expected.reshape(-1)[i].item()!r}")


# ---------------------------------------------------------------- guards shared by the GPU tests
SENT16 = 0x5A5B                   # bf16 1.54e16 as int16: no GEMM of these inputs produces it
SENT32 = 0x5A5B5A5B
GUARD_ROWS = 256


def assert_bits(y, expected):
    """The one assertion of the plain paths: torch.equal against the fp64-derived expectation."""
    msg = bits_mismatch(y, expected)
    assert msg is None, msg


def assert_swiglu(y, ref):
    msg = swiglu_mismatch(y, ref)
    assert msg is None, msg


def sentinel_out(rows, cols, device="cuda"):
    """(buf, y): y = rows [G, G + rows) of an int16 buffer of sentinels, viewed as bf16."""
    g = GUARD_ROWS
    buf = torch.full((g + rows + g, cols), SENT16, dtype=torch.int16, device=device)
    return buf, buf.view(BF16)[g:g + rows]


def assert_untouched(rows, what):
    """``rows``: a slice of a sentinel_out buffer that no kernel may have written."""
    bad = (rows != SENT16).any(dim=1).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows written, first at offset {bad[0].item()}"


# ---------------------------------------------------------------- case lists (part A)
# gemm_wide: (m, n, k, r, splits, variant)
WIDE_M = [1, 64, 65, 128, 129, 192, 193, 256, 300, 384, 385, 512, 640]
WIDE_M_CASES = [(m, 256, 512, 8, s, 1) for m in WIDE_M for s in (1, 3)]
WIDE_BM_CASES = [(m, 256, 512, 8, s, 1 | (bm << 8)) for bm in (64, 128, 192, 256) for m in (65, 300)
                 for s in (1, 2)]
WIDE_VARIANT_CASES = [(129, 256, 1024, 4, s, v) for v in (0, 1, 1 | 32) for s in (1, 3)] + [(2100, 256, 128, 8, 1, 1)]
WIDE_SPLIT_CASES = [(m, n, k, r, s, 1) for m, n, k, r, s in [
    (129, 128, 64, 8, 1), (129, 128, 64, 8, 2),          # splits > K / 64: one slice runs
    (300, 1024, 128, 8, 2), (129, 128, 128, 8, 16),      # 16 asked, 2 run
    (300, 128, 192, 8, 3), (129, 1024, 192, 8, 2),       # uneven: slices of 2 and 1 K-tiles
    (129, 128, 512, 8, 5), (300, 128, 512, 8, 8),        # 5 asked: 4 slices of 2 K-tiles
    (129, 1024, 1024, 4, 16), (300, 128, 1024, 4, 3),
    (129, 128, 4096, 4, 5), (300, 1024, 4096, 4, 8), (129, 128, 4096, 4, 16),
    (256, 256, 14336, 2, 16), (256, 256, 14336, 2, 8)]]
# gemm_sq: (m, n, k, r, splits)
SQ_CASES = [(m, n, k, r, s) for m in (129, 225, 256) for n, k, r, s in [
    (256, 64, 8, 1), (256, 256, 8, 3), (1024, 1024, 4, 16), (256, 4096, 4, 16), (1024, 4096, 4, 3)]]
# gemm_pp: every variant of test_gemm_gpu.test_pp_linear x (m, n, k, r, splits)
PP_VARIANTS = [0, 1, 2, 3, 4, 5, 64, 65, 66, 68, 69]
PP_SHAPES = [(1, 256, 64, 8, 1), (77, 512, 192, 8, 3), (257, 256, 320, 8, 2), (777, 512, 128, 8, 16),
             (256, 256, 4096, 4, 16)]
# gemm_pf: (m, n, k, r, variant); N = 4096 at M = 4100 is 272 tiles on 256 CUs
PF_CASES = [(m, 4096, 128, 8, 0) for m in (1, 255, 256, 257, 4100)] + [(77, 256, 64, 8, 0), (257, 512, 192, 8, 8)]
PF_DYNAMIC_CASES = [(4100, 4096, 128, 8), (300, 512, 192, 8)]
# ops.linear, one shape per branch of gemm.linear: (branch, m, n, k, r).  The first three run a K split (the
# smallest K that still splits); sq is the decode range's unsplit 256 x 256 grid (130 tiles), pp_head the
# decode LM head (N > 65536), torch what no kernel takes (N % 256 above the decode range)
DISPATCH_CASES = [("wide", 64, 256, 4096, 4), ("pp_down", 256, 256, 16384, 2), ("pp", 300, 512, 384, 8),
                  ("pf", 4096, 4096, 128, 8), ("sq", 256, 33280, 128, 8), ("pp_head", 256, 65792, 128, 8),
                  ("torch", 300, 4224, 128, 8)]
DISPATCH_SPLIT = ("wide", "pp_down", "pp")
# ops.linear_swiglu, one shape per branch of gemm.linear_swiglu: (branch, m, inter, k) -- decode gate|up on
# gemm_pp's 128-column tile (128 tiles on 256 CUs) and on its 256-column tile (258 / 129 tiles), gemm_wide,
# medium-M gemm_pp (2 K slices into the SwiGLU reduce) and gemm_pf
SWIGLU_DISPATCH_CASES = [("pp128", 256, 8192, 128), ("pp256", 256, 16512, 128), ("wide", 64, 256, 128),
                         ("pp", 300, 256, 384), ("pf", 4096, 2048, 128)]
# splitk_add_rms_norm: (m, n, k, r, splits) with S == splits
NORM_CASES = [(65, 1024, 128, 8, 2), (65, 4096, 512, 8, 8), (65, 1024, 1024, 4, 16), (129, 4096, 128, 8, 2)]
# part C: partly filled row tiles; (n, k, r, splits)
GUARD_M = [1, 65, 129, 257, 300]
GUARD_SHAPE = (256, 192, 8, 3)
# part E: (m, inter, k)
SWIGLU_WIDE = [(m, 192, 256) for m in WIDE_M] + [(300, i, 256) for i in (64, 128, 1024)] + [(129, 128, 4096)] + \
              [(2100, 128, 256)]                           # prefill M: 9 row tiles
SWIGLU_SQ = [(129, 128, 256), (225, 1024, 256), (256, 128, 4096)]
SWIGLU_PF = [(1, 128, 256), (255, 128, 256), (256, 1024, 256), (257, 1024, 256), (300, 128, 4096), (4100, 128, 256)]
SWIGLU_PP = [(v, m, i, k) for v in (0, 4, 6, 64, 68) for m, i, k in [(77, 128, 256), (257, 1024, 256)]] + \
            [(v, m, i, k) for v in (1, 5, 65) for m, i, k in [(77, 64, 256), (257, 192, 256), (300, 1024, 256)]] + \
            [(64, 256, 128, 4096), (65, 256, 192, 4096)] + \
            [(v, m, 128, 256) for v in (0, 64) for m in (1, 777)] + \
            [(v, m, i, 256) for v in (1, 65) for m, i in ((1, 64), (777, 192))]


def all_int_cases():
    """Every (m, n, k, r, splits) the GPU tests of part A, C and D launch, for the CPU precondition test."""
    out = []
    for c in WIDE_M_CASES + WIDE_BM_CASES + WIDE_VARIANT_CASES + WIDE_SPLIT_CASES:
        out.append(c[:5])
    out += SQ_CASES
    out += PP_SHAPES
    out += [(m, n, k, r, 1) for m, n, k, r, _ in PF_CASES] + [(m, n, k, r, 1) for m, n, k, r in PF_DYNAMIC_CASES]
    out += NORM_CASES
    n, k, r, s = GUARD_SHAPE
    out += [(m, n, k, r, s) for m in GUARD_M] + [(4100, 512, 128, 8, 1), (257, 512, 128, 8, 1)]
    out += [(m, n, k, r, s) for b, m, n, k, r in DISPATCH_CASES for s in (range(2, 17) if b in DISPATCH_SPLIT else (1,))]
    return sorted(set(out))
