"""Bit-exact tests of the hand-written GEMM family (gemm_wide, gemm_sq, gemm_pp, gemm_pf, the
split-K reducers and the fused add + RMSNorm): inputs whose result is known to the last bit, so a
dropped or doubled k, a wrong rounding mode, a slab that loses bits or a store outside the output
shows as a mismatch at a named (m, n) instead of hiding under a 3 % tolerance.

Input forms (built on the CPU by tests/gemm_exact_cases.py, whose preconditions also run without a
GPU in tests/test_exact_cases.py):

  integer   x [M, K] and w [N, K] hold uniform integers in [-r, r].  Every product and every partial
            sum is an integer of magnitude <= K r^2 < 2^24, so f32 accumulation is exact in any
            order, in any MFMA shape and for any K split; the only rounding is the final f32 -> bf16
            store.  Expected: (x.double() @ w.double().T).to(bf16), compared with torch.equal.
            bf16 keeps 8 significant bits, so integers in (256, 512) are 2 apart and every odd one
            is an exact tie: the builder asserts that >= 5 % of a case's outputs are not
            representable and >= 1 % are ties, which makes the comparison a test of
            round-to-nearest-even as well (truncation, round-half-away and double rounding through a
            narrower slab all move some of them).
  slabs     split-K partials are stored as f16 x 2^-6 (csrc/kernels/common.h, DLLM_PART_TYPE 2).
            f16 has an 11-bit significand, so an integer partial p is stored exactly iff
            |p| <= 2^11 = 2048 (p 2^-6 >= 2^-6 is far above the subnormal range).  Before every split
            launch the test computes each slice's partial in fp64 from the launchers' own slice rule
            (kts = ceil(K / 64 / splits) K-tiles per slice, S = ceil(K / 64 / kts) slices) and
            asserts the bound; it also asserts the S the launcher returns.
  selector  x is k rows of a zero matrix with one 1 each, every column used once (a row-permuted
            identity, M >= K); w holds random bf16 bit patterns (both signs, exponents 2^-8 .. 2^8,
            all mantissa bits).  1 w + 0 + ... is exact, so y[row_j, :] == w[:, j] bit for bit: a k
            read twice, never, or from the wrong chunk of a swizzled LDS row shows at that row.  For
            split paths w must survive the slab: (w 2^-6).half() 64 == w, which holds because
            |w| 2^-6 >= 2^-14 (f16's smallest normal) and 8 significant bits fit 11 -- asserted.
  ternary   SwiGLU: x in {-1, 0, 1}, w = [Wg; Wu] in {-1, 0, 1} x 2^-6, K <= 4096.  Every gate / up
            sum is an integer of magnitude <= 256 (asserted) times 2^-6: exact in f32, in bf16 (8
            bits: gemm_pp's two-phase epilogue rounds g and u to bf16, an intended rounding point
            that is the identity on these values) and in the f16 slabs (partials are <= 2048).  One
            fp64 reference silu(g) u serves every SwiGLU path.

Tolerances (only where a transcendental or a division is involved; everything else is torch.equal):

  SwiGLU    rtol = 2^-8 + 2^-12, atol = 1e-30.  2^-8 is half a bf16 ulp, the final store.  silu_f is
            x rcp(1 + __expf(-x)): relative error about |x| 2^-24 plus a few f32 ulp, below 2^-20
            for |g| <= 4; the product with u adds 2^-24.  The 2^-12 term is margin, not a fit.
  RMSNorm   the new residual is bf16(bf16(h) + res) with integer |res| <= 64 -- exact before each
            store, so it is compared bit for bit.  The normed output is compared with an fp64
            RMSNorm of that exact residual at rtol = 2^-8 + 2^-12: half a bf16 ulp for the store plus
            a margin for the f32 rsqrt and the f32 sum of squares (orders above their error, 5 bits
            below an ulp).

Guards (part C): the output is rows [G, G + M) of a larger buffer filled with a sentinel bit
pattern, x and w sit between NaN rows, and the workspace is a view of exactly S M N floats followed
by sentinels.  Every pointer stays inside a live allocation; a store to row M, M + 1, ... of a partly
filled row tile or past the slabs changes a sentinel, a staging read of a guard row that reaches an
accumulator puts a NaN into the output.  The slabs are f16, so all of the workspace past S M N
*halves* must stay untouched too.

Containment (part D): a NaN in row j of x (whole row or one k) makes exactly row j of the output
NaN, an inf at one w[n, k] makes exactly column n non-finite; every other element is bit-identical
to the clean result.  j = M - 1 also covers the masked rows of the last row tile, which the kernels
stage from row M - 1.
"""
import pytest
import torch

import gemm_exact_cases as gx
from distributed_llms_amd import _ext, knobs, ops
from distributed_llms_amd.ops import gemm

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
G = gx.GUARD_ROWS
assert_bits, assert_swiglu, sentinel_out = gx.assert_bits, gx.assert_swiglu, gx.sentinel_out
WS_TAIL = 1 << 16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def launch(kern, x, w, splits=1, mode=0, variant=None, y=None, ws=None, ws_floats=None):
    """One launch of gemm_{wide,sq,pp,pf} through the raw binding -> (y, S).  ``variant`` None: the shipped word."""
    if variant is None:
        variant = {"wide": gemm.WIDE_SPLIT_VARIANT if splits > 1 else gemm.WIDE_VARIANT, "sq": gemm.SQ_VARIANT,
                   "pp": gemm.PP_SCHED2, "pf": 0}[kern]
    m, k = x.shape
    n = w.shape[0]
    kk = _ext.kernels()
    if y is None and mode != 2:
        y = torch.empty(m, n // 2 if mode == 1 else n, dtype=BF, device=x.device)
    yp = y.data_ptr() if y is not None else 0
    if kern == "pf":
        kk.gemm_pf(yp, x.data_ptr(), w.data_ptr(), m, n, k, mode, variant, _stream())
        return y, 1
    if ws is None:
        ws = gemm._workspace(x.device)
        ws_floats = ws.numel()
    s = getattr(kk, "gemm_" + kern)(yp, x.data_ptr(), w.data_ptr(), ws.data_ptr(), ws_floats, m, n, k, splits, mode,
                                    variant, _stream())
    return y, s


def reduce_slabs(ws, s, m, n, y=None):
    if y is None:
        y = torch.empty(m, n, dtype=BF, device=ws.device)
    _ext.kernels().splitk_reduce(y.data_ptr(), ws.data_ptr(), 0, s, m, n, _stream())
    return y


def run_plain(kern, m, n, k, r, splits, variant):
    """Mode 0 and, with a K split, mode 2 -> splitk_reduce: both must equal the expectation."""
    c = gx.int_case(m, n, k, r)
    gx.check_slabs(c, splits)
    x, w = c.x.cuda(), c.w.cuda()
    y, s = launch(kern, x, w, splits, 0, variant)
    if kern != "pf":
        assert s == gx.slice_rule(k, splits)[0]
    assert_bits(y, c.expected)
    if s > 1:
        _, s2 = launch(kern, x, w, splits, 2, variant)
        assert s2 == s
        assert_bits(reduce_slabs(gemm._workspace(x.device), s2, m, n), c.expected)


# ------------------------------------------------------------------ A. integer GEMM, plain mode
@pytest.mark.parametrize("m,n,k,r,splits,variant", gx.WIDE_M_CASES)
def test_wide_row_tiles_from_m(cuda, m, n, k, r, splits, variant):
    """Row tiles 64 / 128 / 192 / 256 as wide_bm picks them from M, full and partly filled, one and
    several row tiles, unsplit and 3 K slices (direct and deferred)."""
    run_plain("wide", m, n, k, r, splits, variant)


@pytest.mark.parametrize("m,n,k,r,splits,variant", gx.WIDE_BM_CASES)
def test_wide_row_tiles_forced(cuda, m, n, k, r, splits, variant):
    """The row-tile override (variant | bm << 8, what knobs.wide_small_bm selects)."""
    run_plain("wide", m, n, k, r, splits, variant)


@pytest.mark.parametrize("m,n,k,r,splits,variant", gx.WIDE_VARIANT_CASES)
def test_wide_variants(cuda, m, n, k, r, splits, variant):
    """Words 0 and 1 (weights nontemporal when unsplit), per-row fragment waits (32), and word 1 at prefill M."""
    run_plain("wide", m, n, k, r, splits, variant)


@pytest.mark.parametrize("m,n,k,r,splits,variant", gx.WIDE_SPLIT_CASES)
def test_wide_k_and_splits(cuda, m, n, k, r, splits, variant):
    """K from one K-tile to 14336, 1 .. 16 slices, uneven last slices and more slices asked than
    K-tiles exist; N of 1 and 8 column tiles."""
    run_plain("wide", m, n, k, r, splits, variant)


@pytest.mark.parametrize("variant", [4])
@pytest.mark.parametrize("m,n,k,r,splits", gx.SQ_CASES)
def test_sq(cuda, m, n, k, r, splits, variant):
    run_plain("sq", m, n, k, r, splits, variant)


@pytest.mark.parametrize("variant", gx.PP_VARIANTS)
@pytest.mark.parametrize("m,n,k,r,splits", gx.PP_SHAPES)
def test_pp(cuda, m, n, k, r, splits, variant):
    run_plain("pp", m, n, k, r, splits, variant)


@pytest.mark.parametrize("m,n,k,r,variant", gx.PF_CASES)
def test_pf(cuda, m, n, k, r, variant):
    """The persistent kernel's static tile walk: fewer tiles than CUs, more tiles than CUs (several
    per workgroup, M = 4100), a tiny grid, and nontemporal stores (variant 8)."""
    run_plain("pf", m, n, k, r, 1, variant)


@pytest.mark.parametrize("m,n,k,r", gx.PF_DYNAMIC_CASES)
def test_pf_dynamic_queue_resets_itself(cuda, m, n, k, r):
    """The per-XCD tile queues (knobs.pf_dynamic): two launches in a row on one stream; the second
    only covers every tile once if the first one's last workgroup reset the heads."""
    c = gx.int_case(m, n, k, r)
    x, w = c.x.cuda(), c.w.cuda()
    with knobs.override(pf_dynamic=True):
        assert gemm.pf_dynamic()
        y1 = gemm.linear_pf(x, w)
        y2 = gemm.linear_pf(x, w)
    assert_bits(y1, c.expected)
    assert_bits(y2, c.expected)


@pytest.fixture
def launches(monkeypatch):
    """Every gemm_* launch the host path makes, as (function, variant), with the launch going through."""
    calls = []
    kk = _ext.kernels()

    class Spy:
        def __getattr__(self, name):
            f = getattr(kk, name)
            if not name.startswith("gemm_"):
                return f

            def launcher(*a):                 # (..., mode, variant, stream) in every gemm_* launcher
                calls.append((name, a[-2]))
                return f(*a)
            return launcher

    spy = Spy()
    monkeypatch.setattr(_ext, "kernels", lambda: spy)
    return calls


def assert_launches(calls, want, count):
    """``want``: None (no launch), or (function, variant or None: whatever the knobs say)."""
    assert [(f, v if want[1] is not None else None) for f, v in calls] == ([want] * count if want else []), calls


@pytest.mark.parametrize("branch,m,n,k,r", gx.DISPATCH_CASES)
def test_dispatcher_shipped_defaults(cuda, launches, branch, m, n, k, r):
    """ops.linear and ops.linear(defer=True) with the shipped knobs, one shape per branch of
    gemm.linear: the decode LM head on gemm_pp, the long-K down projection on split gemm_pp
    (pp_down_min_k), gemm_wide, gemm_sq on its unsplit grid, medium-M gemm_pp, gemm_pf, and F.linear."""
    c = gx.int_case(m, n, k, r)
    x, w = c.x.cuda(), c.w.cuda()
    for s in range(2, 17) if branch in gx.DISPATCH_SPLIT else ():
        gx.check_slabs(c, s)                              # whatever K split the dispatcher picks
    y = ops.linear(x, w)
    d = ops.linear(x, w, defer=True)
    want = {"wide": ("gemm_wide", None), "pp_down": ("gemm_pp", gemm.PP_DOWN_VARIANT),
            "pp": ("gemm_pp", gemm.PP_PREFILL_VARIANT), "pf": ("gemm_pf", None), "sq": ("gemm_sq", None),
            "pp_head": ("gemm_pp", gemm.PP_HEAD_VARIANT), "torch": None}[branch]
    assert_launches(launches, want, 2)
    if branch in gx.DISPATCH_SPLIT:
        assert isinstance(d, gemm.SplitKPartial) and 1 < d.splits <= 16
        d = d.materialize()
    assert_bits(y, c.expected)
    assert_bits(d, c.expected)


@pytest.mark.parametrize("branch,m,inter,k", gx.SWIGLU_DISPATCH_CASES)
def test_swiglu_dispatcher_shipped_defaults(cuda, launches, branch, m, inter, k):
    """ops.linear_swiglu with the shipped knobs, one shape per branch of gemm.linear_swiglu."""
    c = gx.swiglu_case(m, inter, k)
    y = ops.linear_swiglu(c.x.cuda(), c.w.cuda())
    want = {"pp128": ("gemm_pp", gemm.PP_GATE_UP_VARIANT), "pp256": ("gemm_pp", gemm.PP_GATE_UP_VARIANT & ~gemm.PP_BN128),
            "wide": ("gemm_wide", None), "pp": ("gemm_pp", gemm.PP_PREFILL_VARIANT), "pf": ("gemm_pf", None)}[branch]
    assert_launches(launches, want, 1)
    assert y.shape == (m, inter)
    assert_swiglu(y, c.ref)


def norm_reference(new_res, g, eps):
    r = new_res.double()
    return r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * g.double()


def norm_inputs(m, n, seed):
    gen = gx.gen(m, n, seed, 3)
    res = torch.randint(-64, 65, (m, n), generator=gen).to(BF)
    g = (1 + 0.1 * torch.randn(n, generator=gen)).to(BF)
    return res, g


def assert_norm(y, new_res, g, eps):
    ref = norm_reference(new_res, g, eps)
    err = (y.double() - ref).abs()
    bound = gx.SWIGLU_RTOL * ref.abs()
    assert bool((err <= bound).all()), f"normed output: worst err / bound {(err / bound.clamp(min=1e-300)).max().item()}"


@pytest.mark.parametrize("m,n,k,r,splits", gx.NORM_CASES)
def test_splitk_add_rms_norm(cuda, m, n, k, r, splits):
    """Deferred partials + integer residual through splitk_add_rms_norm (S = 2, 8 and the runtime
    loop at 16; N = 1024 and the guard-free N = 4096 form): the new residual is
    bf16(bf16(h) + res) bit for bit, the normed output within half a bf16 ulp + 2^-12 of fp64."""
    c = gx.int_case(m, n, k, r)
    gx.check_slabs(c, splits)
    res0, g = norm_inputs(m, n, splits)
    x, w, res, g = c.x.cuda(), c.w.cuda(), res0.cuda(), g.cuda()
    _, s = launch("wide", x, w, splits, 2, 1)
    assert s == splits
    y = torch.empty(m, n, dtype=BF, device="cuda")
    _ext.kernels().splitk_add_rms_norm(y.data_ptr(), res.data_ptr(), gemm._workspace(x.device).data_ptr(), s, m, n,
                                       g.data_ptr(), 1e-5, _stream())
    new_res = (c.expected.float() + res0.float()).to(BF)
    assert bool(((c.expected.float() + res0.float()).abs() < 2 ** 24).all())
    assert_bits(res, new_res)
    assert_norm(y, res, g, 1e-5)


# ------------------------------------------------------------------ B. selector inputs
SELECTORS = [("wide", 512, k, s, 1) for k in (64, 192, 512) for s in (1, 3)] + \
            [("pp", 512, k, s, v) for k in (64, 192, 512) for s, v in ((1, 64 | 4), (3, 1), (1, 0))] + \
            [("pf", 512, k, 1, 0) for k in (64, 192, 512)] + \
            [("sq", 256, k, s, 4) for k in (64, 256) for s in (1, 2)]


@pytest.mark.parametrize("kern,m,k,splits,variant", SELECTORS)
def test_selector_every_k_position(cuda, kern, m, k, splits, variant):
    """y[row_j, :] == w[:, j] for arbitrary bf16 values: every k position is read exactly once, from
    the right LDS chunk, in every K-tile of every slice."""
    n = 256
    c = gx.selector_case(m, n, k)
    assert bool(gx.survives_slab(c.w).all())                  # split paths: w passes the f16 slab
    x, w = c.x.cuda(), c.w.cuda()
    y, s = launch(kern, x, w, splits, 0, variant)
    assert s == gx.slice_rule(k, splits)[0]
    assert_bits(y, c.expected)
    assert torch.equal(y.view(torch.int16)[c.rows.cuda()], c.expected.cuda().view(torch.int16)[c.rows.cuda()])
    if s > 1:
        launch(kern, x, w, splits, 2, variant)
        assert_bits(reduce_slabs(gemm._workspace(x.device), s, m, n), c.expected)


# ------------------------------------------------------------------ C. guard rows and guard slabs
def guarded(t, fill=float("nan")):
    """t as rows [G, G + M) of a [G + M + G, cols] device buffer filled with ``fill``."""
    buf = torch.full((G + t.shape[0] + G, t.shape[1]), fill, dtype=t.dtype, device="cuda")
    buf[G:G + t.shape[0]] = t
    return buf[G:G + t.shape[0]]


def assert_guards(buf, m, what):
    gx.assert_untouched(buf[:G], f"{what}: rows before the output")
    bad = (buf[G + m:] != gx.SENT16).any(dim=1).nonzero()
    assert bad.numel() == 0, f"{what}: store to row M + {bad[0].item()} (M = {m})"


def sentinel_ws(floats):
    return torch.full((floats + WS_TAIL,), gx.SENT32, dtype=torch.int32, device="cuda")


def assert_ws(ws, s, m, n):
    # the slabs are f16: S M N elements end half way through the S M N floats the launcher was given
    assert bool((ws[s * m * n // 2:] == gx.SENT32).all()), "store past the S M N f16 slab elements"


@pytest.mark.parametrize("m", gx.GUARD_M)
@pytest.mark.parametrize("kern,variant", [("wide", 1), ("wide", 1 | (64 << 8)), ("wide", 1 | (128 << 8)), ("sq", 4),
                                          ("pp", 64 | 4), ("pp", 1)])
def test_guard_rows_and_slabs(cuda, kern, variant, m):
    """Partly filled row tiles (for gemm_wide also the forced 64- and 128-row tiles): mode 0, mode 2 + splitk_reduce and splitk_add_rms_norm write nothing
    outside [G, G + M) x N and the S M N slab elements, and read no guard row into a result."""
    n, k, r, splits = gx.GUARD_SHAPE
    c = gx.int_case(m, n, k, r)
    gx.check_slabs(c, splits)
    x, w = guarded(c.x), guarded(c.w)
    buf, y = sentinel_out(m, n)
    launch(kern, x, w, 1, 0, variant, y=y)
    assert_bits(y, c.expected)
    assert_guards(buf, m, "mode 0")
    # split: direct (the launcher reduces), then deferred into splitk_reduce and the fused norm
    s_want = gx.slice_rule(k, splits)[0]
    ws = sentinel_ws(s_want * m * n)
    buf, y = sentinel_out(m, n)
    _, s = launch(kern, x, w, splits, 0, variant, y=y, ws=ws, ws_floats=s_want * m * n)
    assert s == s_want
    assert_bits(y, c.expected)
    assert_guards(buf, m, "split mode 0")
    assert_ws(ws, s, m, n)
    ws = sentinel_ws(s * m * n)
    launch(kern, x, w, splits, 2, variant, ws=ws, ws_floats=s * m * n)
    buf, y = sentinel_out(m, n)
    reduce_slabs(ws, s, m, n, y=y)
    assert_bits(y, c.expected)
    assert_guards(buf, m, "splitk_reduce")
    assert_ws(ws, s, m, n)
    res0, g = norm_inputs(m, n, 1)
    rbuf, res = sentinel_out(m, n)
    res.copy_(res0)
    buf, y = sentinel_out(m, n)
    _ext.kernels().splitk_add_rms_norm(y.data_ptr(), res.data_ptr(), ws.data_ptr(), s, m, n, g.cuda().data_ptr(),
                                       1e-5, _stream())
    assert_bits(res, (c.expected.float() + res0.float()).to(BF))
    assert_norm(y, res, g.cuda(), 1e-5)
    assert_guards(rbuf, m, "splitk_add_rms_norm residual")
    assert_guards(buf, m, "splitk_add_rms_norm output")
    assert_ws(ws, s, m, n)


@pytest.mark.parametrize("m", [257, 4100])
def test_pf_guard_rows(cuda, m):
    """gemm_pf drops the rows past M of its last row tile (plain and SwiGLU stores)."""
    c = gx.int_case(m, 512, 128, 8)
    buf, y = sentinel_out(m, 512)
    launch("pf", guarded(c.x), guarded(c.w), 1, 0, 0, y=y)
    assert_bits(y, c.expected)
    assert_guards(buf, m, "gemm_pf mode 0")
    sc = gx.swiglu_case(m, 256, 128)
    buf, y = sentinel_out(m, 256)
    launch("pf", guarded(sc.x), guarded(sc.w), 1, 1, 0, y=y)
    assert_swiglu(y, sc.ref)
    assert_guards(buf, m, "gemm_pf mode 1")


# ------------------------------------------------------------------ D. NaN / inf containment
CONTAIN = [("wide", 1, 1), ("wide", 3, 1), ("sq", 1, 4), ("sq", 3, 4), ("pp", 1, 64 | 4), ("pp", 3, 1), ("pf", 1, 0)]
CONTAIN_K = 70                                            # second K-tile; the second of 3 slices


@pytest.mark.parametrize("kern,splits,variant", CONTAIN)
def test_nan_and_inf_stay_in_their_row_and_column(cuda, kern, splits, variant):
    m, (n, k, r, _) = 129, gx.GUARD_SHAPE
    c = gx.int_case(m, n, k, r)
    gx.check_slabs(c, splits)
    x, w, exp = c.x.cuda(), c.w.cuda(), c.expected.cuda()
    rows = torch.arange(m, device="cuda")
    for j in (0, m - 1):
        for whole in (True, False):
            xp = x.clone()
            if whole:
                xp[j] = float("nan")
            else:
                xp[j, CONTAIN_K] = float("nan")
            y, _ = launch(kern, xp, w, splits, 0, variant)
            assert bool(torch.isnan(y[j]).all()), (j, whole)
            assert_bits(y[rows != j], exp[rows != j])
    col = 131
    wp = w.clone()
    wp[col, CONTAIN_K] = float("inf")
    y, _ = launch(kern, x, wp, splits, 0, variant)
    cols = torch.arange(n, device="cuda")
    assert not bool(torch.isfinite(y[:, col]).any())
    assert_bits(y[:, cols != col], exp[:, cols != col])


@pytest.mark.parametrize("kern,variant", [("wide", 1), ("sq", 4), ("pp", 1)])
def test_nan_row_through_fused_norm(cuda, kern, variant):
    """GEMM (mode 2) -> splitk_add_rms_norm: residual and normed row j are NaN, every other row is
    bit-identical to the clean run."""
    m, (n, k, r, splits) = 129, gx.GUARD_SHAPE
    c = gx.int_case(m, n, k, r)
    gx.check_slabs(c, splits)
    res0, g = norm_inputs(m, n, 2)
    g = g.cuda()
    ws = gemm._workspace(torch.device("cuda", torch.cuda.current_device()))

    def run(x):
        _, s = launch(kern, x, c.w.cuda(), splits, 2, variant)
        res = res0.cuda()
        y = torch.empty(m, n, dtype=BF, device="cuda")
        _ext.kernels().splitk_add_rms_norm(y.data_ptr(), res.data_ptr(), ws.data_ptr(), s, m, n, g.data_ptr(), 1e-5,
                                           _stream())
        return y, res

    y0, r0 = run(c.x.cuda())
    assert_bits(r0, (c.expected.float() + res0.float()).to(BF))
    rows = torch.arange(m, device="cuda")
    for j in (0, m - 1):
        for whole in (True, False):
            xp = c.x.cuda()
            if whole:
                xp[j] = float("nan")
            else:
                xp[j, CONTAIN_K] = float("nan")
            y, res = run(xp)
            assert bool(torch.isnan(y[j]).all()) and bool(torch.isnan(res[j]).all()), (j, whole)
            assert_bits(res[rows != j], r0[rows != j])
            assert_bits(y[rows != j], y0[rows != j])


# ------------------------------------------------------------------ E. SwiGLU paths
def run_swiglu(kern, m, inter, k, splits, variant):
    c = gx.swiglu_case(m, inter, k)
    y, s = launch(kern, c.x.cuda(), c.w.cuda(), splits, 1, variant)
    if kern != "pf":
        assert s == gx.slice_rule(k, splits)[0]
    assert y.shape == (m, inter)
    assert_swiglu(y, c.ref)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("m,inter,k", gx.SWIGLU_WIDE)
def test_wide_swiglu(cuda, m, inter, k, splits):
    """gemm_wide's fused epilogue (64-column gate / up tiles; I = 64, 128, 192, 1024) at every M edge
    of part A and at prefill M (9 row tiles), and 2 K slices into the SwiGLU reduce."""
    run_swiglu("wide", m, inter, k, splits, 33 if splits == 1 else 1)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("m,inter,k", gx.SWIGLU_SQ)
def test_sq_swiglu(cuda, m, inter, k, splits):
    run_swiglu("sq", m, inter, k, splits, 4)


@pytest.mark.parametrize("variant", [0, 8])
@pytest.mark.parametrize("m,inter,k", gx.SWIGLU_PF)
def test_pf_swiglu(cuda, m, inter, k, variant):
    run_swiglu("pf", m, inter, k, 1, variant)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("variant,m,inter,k", gx.SWIGLU_PP)
def test_pp_swiglu(cuda, variant, m, inter, k, splits):
    """gemm_pp's two-phase epilogue rounds gate and up to bf16 before the SiLU -- an intended
    rounding point, the identity on these inputs (|integer| <= 256) -- so the same reference and
    tolerance hold; 128- and 256-column tiles, both schedules, and the split SwiGLU reduce."""
    run_swiglu("pp", m, inter, k, splits, variant)
