"""Bit-exact tests of the FP8 (W8A8) family: gemm_wide_fp8 (the FP8 instantiation of the wide K
loop, ktile8, and the SCALED epilogue), moe_wide_gemm_fp8, quant_fp8_rows and the norm kernels' fp8
epilogue.  Operands are built directly as e4m3 bytes with hand-chosen f32 scales
(tests/fp8_exact_cases.py, whose preconditions and mutants run without a GPU in
tests/test_fp8_cases.py), so the GEMM is tested without the quantizer in front of it, and a
fragment read from the wrong LDS chunk, a scale read one row off, a K-tile lost at a split boundary
or a store outside the output shows as a mismatch at a named (m, n) instead of hiding under the
5-e4m3-step tolerance of test_quant_gpu.py.

Input forms:

  integer   xq [M, K] and wq [N, K] hold uniform integers in [-r, r], r <= 8.  e4m3 has 4
            significant bits, so it holds every integer up to 16 exactly.  Every product and every
            partial sum is an integer of magnitude <= r^2 K <= 64 K < 2^24 (K <= 14336): exact in f32
            in any order, and in v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 scales.  The
            scales are powers of two, sa[m] = 2^((m mod 5) - 2), sb[n] = 2^((n mod 7) - 3): distinct
            along both axes (a scale read one row or column off is wrong by a factor >= 2), and
            they move no rounding boundary, so the rounded (>= 5 %) and tie (>= 1 %) shares are
            asserted on the integer accumulator and the comparison pins round-to-nearest-even of
            the bf16 store.  Expected: bf16(acc sa[m] sb[n]) from fp64, torch.equal.  (r = 8 except
            where a K slice is deeper than 256: r = 4 at K = 1024 in 3 slices and r = 2 at K =
            14336, which keeps every slice's partial inside the slab's 11 bits.)
  slabs     a split launch stores each slice's *scaled* partial p sa sb as f16 x 2^-6.  p is an
            integer with |p| <= 2048 = 2^11 (asserted per slice from the launcher's slice rule on
            128-wide K-tiles, slice_rule(K / 2, splits)), which f16's 11-bit significand holds; the
            power-of-two factor 2^-6 sa sb lies in [2^-11, 2^-2], so the lowest bit of the stored
            value is >= 2^-11, far above f16's subnormal step 2^-24, and its magnitude is <= 2^9.
            The builder asserts the identity f16(v 2^-6) 64 == v on every slice directly.
  general   the same integers with random full-mantissa f32 scales in [2^-6, 2^2].  The epilogue
            computes v * (s * sbn): two f32 multiplies and no addition, so nothing can contract
            into an FMA, and the result is reproduced exactly in numpy float32:
            bf16(f32(f32(acc) f32(sa[m] sb[n]))).  Unsplit only: the f16 slab would be a third
            rounding point, and the power-of-two form covers it.
  selector  xq is a row-permuted identity (one 0x38 = 1.0 per used row, M >= K), wq holds random
            e4m3 bit patterns over every code but NaN and -0, subnormals included, scales are 1:
            y[rows[j], :] == bf16(wq[:, j]) bit for bit.  Every finite e4m3 value is exact in bf16 (4
            of 8 bits) and, times 2^-6, in f16 (>= 2^-15 with 4 bits) -- asserted.  This pins ktile8's
            k map: chunks 2 fq and 2 fq + 1 of the swizzled LDS row, the same map for A and B.
  ternary   SwiGLU: xq and wq = [Wg; Wu] in {-1, 0, 1}, sb = 2^-6, sa = 1, |sum| <= 256 (asserted),
            reference silu(g) u in fp64 at the project's SWIGLU_RTOL / SWIGLU_ATOL (derived in
            test_gemm_exact.py; g and u themselves are exact).

quant_fp8_rows is compared bit for bit with quantize_rows_ref on rows made of the conversion's
edges: one element 448 c (c a power of two, so scale = c and x / scale is exact) and c times every
e4m3 midpoint (ties, which must go to the even code), the subnormal range, +-0 and 446; K at every
MAXV dispatch edge.  End to end, bf16 rows of integers times a power of two with one +-448 c element
quantize to exactly those integers, so quant.linear_fp8 must equal the fp64 product rounded to bf16.

Non-finite inputs: a row with a NaN or Inf element gets a non-finite scale (ops/quant.py), so its
outputs are non-finite and every other row is bit-identical to the clean run.

No tolerance is introduced here: everything is torch.equal except the SwiGLU and normed-row
comparisons, which use SWIGLU_RTOL / SWIGLU_ATOL exactly as test_gemm_exact.py does.
"""
import pytest
import torch

import fp8_exact_cases as fx
import gemm_exact_cases as gx
from distributed_llms_amd import _ext, ops
from distributed_llms_amd.ops import gemm, moe, quant

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
G = gx.GUARD_ROWS
assert_bits, assert_swiglu, sentinel_out, assert_untouched = gx.assert_bits, gx.assert_swiglu, gx.sentinel_out, gx.assert_untouched
WS_TAIL = 1 << 16
SENT8 = 0x5A


def _stream():
    return torch.cuda.current_stream().cuda_stream


def launch(xq, sa, wq, sb, splits=1, mode=0, variant=1, y=None, ws=None, ws_floats=None):
    """One launch of gemm_wide_fp8 through the raw binding -> (y, S).  xq / wq: uint8 e4m3 bytes."""
    m, k = xq.shape
    n = wq.shape[0]
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and wq.shape[1] == k
    assert sa.dtype == torch.float32 and sb.dtype == torch.float32 and sa.numel() == m and sb.numel() == n
    assert xq.is_contiguous() and wq.is_contiguous() and sa.is_contiguous() and sb.is_contiguous()
    if y is None and mode != 2:
        y = torch.empty(m, n // 2 if mode == 1 else n, dtype=BF, device=xq.device)
    if ws is None:
        ws = gemm._workspace(xq.device)
        ws_floats = ws.numel()
    s = _ext.kernels().gemm_wide_fp8(y.data_ptr() if y is not None else 0, xq.data_ptr(), sa.data_ptr(), wq.data_ptr(),
                                     sb.data_ptr(), ws.data_ptr(), ws_floats, m, n, k, splits, mode, variant, _stream())
    return y, s


def reduce_slabs(ws, s, m, n, y=None):
    if y is None:
        y = torch.empty(m, n, dtype=BF, device=ws.device)
    _ext.kernels().splitk_reduce(y.data_ptr(), ws.data_ptr(), 0, s, m, n, _stream())
    return y


def run_int(m, n, k, r, splits, variant):
    """Mode 0 and, with a K split, mode 2 -> splitk_reduce: both must equal the expectation."""
    c = fx.int_case(m, n, k, r)
    fx.check_slabs(c, splits)
    xq, sa, wq, sb = c.xq.cuda(), c.sa.cuda(), c.wq.cuda(), c.sb.cuda()
    y, s = launch(xq, sa, wq, sb, splits, 0, variant)
    assert s == gx.slice_rule(k // 2, splits)[0]
    assert_bits(y, c.expected)
    if s > 1:
        _, s2 = launch(xq, sa, wq, sb, splits, 2, variant)
        assert s2 == s
        assert_bits(reduce_slabs(gemm._workspace(xq.device), s2, m, n), c.expected)


# ------------------------------------------------------------------ 1-3. integer GEMM
@pytest.mark.parametrize("m,n,k,r,splits,variant", fx.ROW_TILE_CASES)
def test_row_tiles(cuda, m, n, k, r, splits, variant):
    """Row tiles 64 / 128 / 192 / 256 as wide_bm picks them from M and forced (variant | bm << 8),
    full and partly filled, unsplit and 2 K slices (3 asked), direct and deferred."""
    run_int(m, n, k, r, splits, variant)


@pytest.mark.parametrize("m,n,k,r,splits,variant", fx.VARIANT_CASES)
def test_variants(cuda, m, n, k, r, splits, variant):
    """Variant 1 (non-temporal weights when unsplit), 4 (plain) and 4 | 64, the grouped row-tile
    order: 9 row tiles at M = 2100 (a partial last group of 8), 10 at M = 2309 with 3 column tiles."""
    run_int(m, n, k, r, splits, variant)


@pytest.mark.parametrize("m,n,k,r,splits,variant", fx.SPLIT_CASES)
def test_k_and_splits(cuda, m, n, k, r, splits, variant):
    """One K-tile; uneven slices (2 and 1 K-tiles); one tile per slice; more slices asked than
    K-tiles exist; K = 14336 in 7 slices of 16 K-tiles."""
    run_int(m, n, k, r, splits, variant)


# ------------------------------------------------------------------ 4. general scales
@pytest.mark.parametrize("m,n,k", fx.GENERAL_CASES)
def test_general_scales(cuda, m, n, k):
    c = fx.int_case(m, n, k, 8, "general")
    y, s = launch(c.xq.cuda(), c.sa.cuda(), c.wq.cuda(), c.sb.cuda(), 1, 0, 1)
    assert s == 1
    assert_bits(y, c.expected)


# ------------------------------------------------------------------ 5. selector
@pytest.mark.parametrize("k,splits,variant", fx.SELECTOR_CASES)
def test_selector_every_k_position(cuda, k, splits, variant):
    """y[row_j, :] == bf16(wq[:, j]) for arbitrary e4m3 codes: every k is read exactly once, from the
    right chunk of the swizzled LDS row, under 64-, 128- and 256-row tiles, unsplit and split."""
    m, n = k, 128
    c = fx.selector_case(m, n, k)
    xq, sa, wq, sb = c.xq.cuda(), c.sa.cuda(), c.wq.cuda(), c.sb.cuda()
    y, s = launch(xq, sa, wq, sb, splits, 0, variant)
    assert s == gx.slice_rule(k // 2, splits)[0]
    assert_bits(y, c.expected)
    rows = c.rows.cuda()
    assert torch.equal(y.view(torch.int16)[rows], c.expected.cuda().view(torch.int16)[rows])       # signs of zeros too
    if s > 1:
        launch(xq, sa, wq, sb, splits, 2, variant)
        assert_bits(reduce_slabs(gemm._workspace(xq.device), s, m, n), c.expected)


def moe_launch(y, xq, gather, wq, counts, offsets, e, n, k, mode, sa, wscale):
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and wq.shape == (e, n, k) and xq.shape[1] == k
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int32 and counts.numel() == e and offsets.numel() == e + 1
    assert sa.dtype == torch.float32 and wscale.dtype == torch.float32 and wscale.shape == (e, n)
    slots = int(offsets[e].item())
    assert sa.numel() == slots and y.shape == (slots, n // 2 if mode == 1 else n)
    if gather is not None:
        assert gather.dtype == torch.int32 and gather.numel() == slots and int(gather.max().item()) < xq.shape[0]
    else:
        assert xq.shape[0] >= slots
    _ext.kernels().moe_wide_gemm_fp8(y.data_ptr(), xq.data_ptr(), gather.data_ptr() if gather is not None else 0,
                                     wq.data_ptr(), counts.data_ptr(), offsets.data_ptr(), e, n, k, mode, sa.data_ptr(),
                                     wscale.data_ptr(), _stream())


@pytest.mark.parametrize("k", [256, 512])
def test_selector_through_the_grouped_kernel(cuda, k):
    """The same selector through moe_wide_gemm_fp8 with one expert and no gather (128-row chunks)."""
    m, n = k, 128
    c = fx.selector_case(m, n, k)
    counts = torch.tensor([m], dtype=torch.int32, device="cuda")
    offsets = torch.tensor([0, m], dtype=torch.int32, device="cuda")
    buf, y = sentinel_out(m, n)
    moe_launch(y, c.xq.cuda(), None, c.wq.cuda().reshape(1, n, k), counts, offsets, 1, n, k, 0, c.sa.cuda(),
               c.sb.cuda().reshape(1, n))
    assert_bits(y, c.expected)
    assert_untouched(buf[:G], "rows before slot 0")
    assert_untouched(buf[G + m:], "rows past the last slot")


# ------------------------------------------------------------------ 6. SwiGLU
@pytest.mark.parametrize("m,inter,k,splits,variant", fx.SWIGLU_CASES)
def test_swiglu(cuda, m, inter, k, splits, variant):
    """The scaled SwiGLU epilogue (gate / up column scales sb[c] and sb[I + c]) at the row-tile
    edges, I = 64 and 192, 2 K slices into the SwiGLU reduce, and the grouped row-tile order."""
    c = fx.swiglu_case(m, inter, k)
    y, s = launch(c.xq.cuda(), c.sa.cuda(), c.wq.cuda(), c.sb.cuda(), splits, 1, variant)
    assert s == gx.slice_rule(k // 2, splits)[0]
    assert y.shape == (m, inter)
    assert_swiglu(y, c.ref)


# ------------------------------------------------------------------ 7. guards
def guarded(t, fill):
    """t as rows [G, G + M) of a [G + M + G, ...] device buffer filled with ``fill``."""
    buf = torch.full((G + t.shape[0] + G, *t.shape[1:]), fill, dtype=t.dtype, device="cuda")
    buf[G:G + t.shape[0]] = t
    return buf[G:G + t.shape[0]]


def assert_guards(buf, m, what):
    assert_untouched(buf[:G], f"{what}: rows before the output")
    bad = (buf[G + m:] != gx.SENT16).any(dim=1).nonzero()
    assert bad.numel() == 0, f"{what}: store to row M + {bad[0].item()} (M = {m})"


def sentinel_ws(floats):
    return torch.full((floats + WS_TAIL,), gx.SENT32, dtype=torch.int32, device="cuda")


def assert_ws(ws, s, m, n):
    # the slabs are f16: S M N elements end half way through the S M N floats the launcher was given
    assert bool((ws[s * m * n // 2:] == gx.SENT32).all()), "store past the S M N f16 slab elements"


@pytest.mark.parametrize("m", gx.GUARD_M)
@pytest.mark.parametrize("variant", [1, 1 | (64 << 8), 1 | (128 << 8)])
def test_guard_rows_and_slabs(cuda, variant, m):
    """Partly filled row tiles: mode 0, split mode 0 and mode 2 + splitk_reduce write nothing outside
    [G, G + M) x N and the S M N slab elements and read no guard into a result.  xq and wq sit
    between rows of 0x7F (e4m3 NaN) bytes, sa and sb between NaN floats."""
    n, k, r, splits = fx.GUARD_SHAPE
    c = fx.int_case(m, n, k, r)
    fx.check_slabs(c, splits)
    nan = float("nan")
    xq, wq, sa, sb = guarded(c.xq, fx.NAN_BYTE), guarded(c.wq, fx.NAN_BYTE), guarded(c.sa, nan), guarded(c.sb, nan)
    buf, y = sentinel_out(m, n)
    launch(xq, sa, wq, sb, 1, 0, variant, y=y)
    assert_bits(y, c.expected)
    assert_guards(buf, m, "mode 0")
    s_want = gx.slice_rule(k // 2, splits)[0]
    assert s_want == 2
    ws = sentinel_ws(s_want * m * n)
    buf, y = sentinel_out(m, n)
    _, s = launch(xq, sa, wq, sb, splits, 0, variant, y=y, ws=ws, ws_floats=s_want * m * n)
    assert s == s_want
    assert_bits(y, c.expected)
    assert_guards(buf, m, "split mode 0")
    assert_ws(ws, s, m, n)
    ws = sentinel_ws(s * m * n)
    launch(xq, sa, wq, sb, splits, 2, variant, ws=ws, ws_floats=s * m * n)
    buf, y = sentinel_out(m, n)
    reduce_slabs(ws, s, m, n, y=y)
    assert_bits(y, c.expected)
    assert_guards(buf, m, "splitk_reduce")
    assert_ws(ws, s, m, n)


# ------------------------------------------------------------------ 8. grouped FP8 kernel
@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("counts,top_k", fx.MOE_ROUTINGS)
def test_grouped_fp8_slot_expert_and_scale_mapping(cuda, counts, top_k, mode, gathered):
    """Every slot is multiplied by its own expert's weights, by the row gather names (or its own
    row), by its own per-slot scale (slot order, not token order) and by its expert's per-channel
    scales; experts with no rows, 64- and 128-row tiles, chunks that end inside a segment; nothing
    outside the slot rows is written."""
    rt = fx.routing(counts, top_k)
    e = len(counts)
    if mode == 0:
        n, k = fx.MOE_INT_DIMS[gathered]
        cols = n
    else:
        inter, k = fx.MOE_SWIGLU_DIMS[gathered]
        n, cols = 2 * inter, inter
    c = fx.moe_case(counts, top_k, n, k, gathered, mode)
    gather = rt.gather.cuda() if gathered else None
    buf, y = sentinel_out(rt.slots, cols)
    moe_launch(y, c.xq.cuda(), gather, c.wq.cuda(), rt.counts.cuda(), rt.offsets.cuda(), e, n, k, mode, c.sa.cuda(),
               c.wscale.cuda())
    if mode == 0:
        assert_bits(y, c.expected)
    else:
        assert_swiglu(y, c.ref)
    assert_untouched(buf[:G], "rows before slot 0")
    assert_untouched(buf[G + rt.slots:], "rows past the last slot")


@pytest.mark.parametrize("lo,hi", [(2, 6), (0, 2)])
def test_grouped_fp8_local_expert_range(cuda, lo, hi):
    """counts / offsets advanced to experts [lo, hi) with their weights and scales only: the slots of
    every other expert keep their sentinel."""
    counts, top_k = fx.MOE_ROUTINGS[0]
    rt = fx.routing(counts, top_k)
    n, k = fx.MOE_INT_DIMS[True]
    c = fx.moe_case(counts, top_k, n, k, True, 0)
    cnt, off = rt.counts.cuda(), rt.offsets.cuda()
    wq, wscale = c.wq[lo:hi].contiguous().cuda(), c.wscale[lo:hi].contiguous().cuda()
    xq, sa, gather = c.xq.cuda(), c.sa.cuda(), rt.gather.cuda()
    buf, y = sentinel_out(rt.slots, n)
    assert sa.numel() == rt.slots and gather.numel() == rt.slots and int(gather.max().item()) < xq.shape[0]
    _ext.kernels().moe_wide_gemm_fp8(y.data_ptr(), xq.data_ptr(), gather.data_ptr(), wq.data_ptr(), cnt.data_ptr() + 4 * lo,
                                     off.data_ptr() + 4 * lo, hi - lo, n, k, 0, sa.data_ptr(), wscale.data_ptr(), _stream())
    a, b = rt.offsets[lo].item(), rt.offsets[hi].item()
    assert_bits(y[a:b], c.expected[a:b])
    assert_untouched(buf[:G + a], "slots of the experts below the local range")
    assert_untouched(buf[G + b:], "slots of the experts above the local range")


# ------------------------------------------------------------------ 9. end to end through quant.linear_fp8
def norm_reference(new_res, g, eps):
    r = new_res.double()
    return r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * g.double()


def assert_norm(y, new_res, g, eps):
    ref = norm_reference(new_res, g, eps)
    err = (y.double() - ref).abs()
    bound = gx.SWIGLU_RTOL * ref.abs()
    assert bool((err <= bound).all()), f"normed output: worst err / bound {(err / bound.clamp(min=1e-300)).max().item()}"


@pytest.mark.parametrize("m,n,k,r", fx.E2E_CASES)
def test_quantize_then_linear_fp8_is_the_exact_product(cuda, m, n, k, r):
    """quantize_rows / quantize_weight return exactly the builder's integer codes and power-of-two
    scales; linear_fp8 (its own plan: unsplit, or 4 slices under 128-row tiles at M = 200) equals
    bf16 of the fp64 product.  At M = 200 also deferred into fused_add_rms_norm: the new residual bit
    for bit, the normed row at SWIGLU_RTOL."""
    c = fx.e2e_case(m, n, k, r)
    s_plan, bm = quant.fp8_plan(m, n, k)
    if m == 200:
        assert bm == 128 and s_plan > 1, (s_plan, bm)
    fx.check_slabs_of(c.xq, c.wq, c.c, c.d, s_plan)
    x = c.x.cuda()
    q, s = quant.quantize_rows(x)
    assert torch.equal(q.view(torch.uint8).cpu(), c.xq) and torch.equal(s.cpu(), c.c)
    fw = quant.quantize_weight(c.w.cuda())
    assert torch.equal(fw.q.view(torch.uint8).cpu(), c.wq) and torch.equal(fw.scale.cpu(), c.d)
    assert_bits(quant.linear_fp8(x, fw), c.expected)
    if s_plan > 1:
        part = quant.linear_fp8(x, fw, defer=True)
        assert isinstance(part, gemm.SplitKPartial) and part.splits == gx.slice_rule(k // 2, s_plan)[0]
        gen = gx.gen(m, n, 3)
        res0 = torch.randint(-64, 65, (m, n), generator=gen).to(BF)
        g = (1 + 0.1 * torch.randn(n, generator=gen)).to(BF).cuda()
        exact = c.expected.double() + res0.double()
        assert torch.equal((c.expected.float() + res0.float()).double(), exact)          # the f32 add is exact
        y, res = ops.fused_add_rms_norm(part, res0.cuda(), g, 1e-5)
        assert_bits(res, exact.to(BF))
        assert_norm(y, res, g, 1e-5)


# ------------------------------------------------------------------ 10. quant_fp8_rows at its edges
@pytest.mark.parametrize("k", fx.QUANT_K)
@pytest.mark.parametrize("m", [1, 3])
def test_quant_rows_edges(cuda, m, k):
    """Every MAXV dispatch edge (16392: the re-read path); rows of e4m3 ties, subnormals, +-0 and
    446; q and scale between sentinel rows.  Bit for bit against quantize_rows_ref."""
    c = fx.quant_rows_case(m, k)
    x = c.x.cuda()
    qbuf = torch.full((G + m + G, k), SENT8, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((G + m + G,), gx.SENT32, dtype=torch.int32, device="cuda")
    q, s = qbuf[G:G + m], sbuf[G:G + m]
    _ext.kernels().quant_fp8_rows(q.data_ptr(), s.data_ptr(), x.data_ptr(), m, k, _stream())
    assert torch.equal(s.view(torch.float32).cpu(), c.scale)
    bad = (q.cpu() != c.q).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} codes differ; first at {bad[0].tolist()}: x / scale = "
                              f"{(c.x[tuple(bad[0])].double() / c.scale[bad[0][0]].double()).item()!r}, got "
                              f"{q[tuple(bad[0])].item():#x}, expected {c.q[tuple(bad[0])].item():#x}")
    assert bool((qbuf[:G] == SENT8).all()) and bool((qbuf[G + m:] == SENT8).all()), "q rows outside [0, M) written"
    assert bool((sbuf[:G] == gx.SENT32).all()) and bool((sbuf[G + m:] == gx.SENT32).all()), "scales outside [0, M) written"


@pytest.mark.parametrize("hidden", [136, 2056, 8200])
def test_norm_epilogue_on_edge_rows(cuda, hidden):
    """rms_norm / fused_add_rms_norm with quant_out on the edge rows (weight of ones): the f32
    rsqrt and eps keep the normed values from being chosen exactly, so this is the identity of
    test_quant_gpu.py -- the fused output is the quantization of the bf16 output -- held against the
    CPU reference quantizer as well."""
    m = 3
    x = fx.quant_rows_case(m, hidden).x.cuda()
    w = torch.ones(hidden, dtype=BF, device="cuda")
    a = ops.rms_norm(x, w, 1e-5, quant_out=True)
    y = ops.rms_norm(x, w, 1e-5)
    q, s = quant.quantize_rows(y)
    qr, sr = quant.quantize_rows_ref(y.cpu())
    assert torch.equal(a.q.view(torch.uint8), q.view(torch.uint8)) and torch.equal(a.scale, s)
    assert torch.equal(a.q.view(torch.uint8).cpu(), qr.view(torch.uint8)) and torch.equal(a.scale.cpu(), sr)
    res = fx.quant_rows_case(m, hidden, 1).x.cuda()
    r1, r2 = res.clone(), res.clone()
    a, r1 = ops.fused_add_rms_norm(x, r1, w, 1e-5, quant_out=True)
    y, r2 = ops.fused_add_rms_norm(x, r2, w, 1e-5)
    qr, sr = quant.quantize_rows_ref(y.cpu())
    assert torch.equal(r1, r2)
    assert torch.equal(a.q.view(torch.uint8).cpu(), qr.view(torch.uint8)) and torch.equal(a.scale.cpu(), sr)


# ------------------------------------------------------------------ non-finite inputs
NF_M, NF_COL = 37, 70


def assert_contract(s, q, s0, q0, j, kind):
    msg = fx.nonfinite_contract(s, q, s0, q0, j, kind)
    assert msg is None, msg


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("k", [256, 8200, 16392])
def test_nonfinite_row_quantize_rows(cuda, k, kind):
    x = fx.quant_rows_case(NF_M, k).x.cuda()
    q0, s0 = quant.quantize_rows(x)
    for j in (0, NF_M - 1):
        q, s = quant.quantize_rows(fx.poison(x, j, NF_COL, kind))
        assert_contract(s, q, s0, q0, j, kind)


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("hidden", [256, 8200])
def test_nonfinite_row_norm_epilogues(cuda, hidden, kind):
    x = fx.quant_rows_case(NF_M, hidden).x.cuda()
    res = fx.quant_rows_case(NF_M, hidden, 1).x.cuda()
    w = (1 + 0.1 * torch.randn(hidden, generator=gx.gen(hidden, 7))).to(BF).cuda()
    a0 = ops.rms_norm(x, w, 1e-5, quant_out=True)
    b0, r0 = ops.fused_add_rms_norm(x, res.clone(), w, 1e-5, quant_out=True)
    keep = torch.arange(NF_M, device="cuda")
    for j in (0, NF_M - 1):
        xp = fx.poison(x, j, NF_COL, kind)
        a = ops.rms_norm(xp, w, 1e-5, quant_out=True)
        assert_contract(a.scale, a.q, a0.scale, a0.q, j, kind)
        b, r = ops.fused_add_rms_norm(xp, res.clone(), w, 1e-5, quant_out=True)
        assert_contract(b.scale, b.q, b0.scale, b0.q, j, kind)
        assert_bits(r[keep != j], r0[keep != j])


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("splits", [1, 2])
def test_nonfinite_row_through_linear_fp8(cuda, splits, kind):
    """Row j is entirely non-finite, every other element bit-identical; j = M - 1 also covers the
    masked rows of the last row tile, which the kernel stages from row M - 1."""
    m, n, k = 65, 256, 512
    c = fx.e2e_case(m, n, k)
    fx.check_slabs_of(c.xq, c.wq, c.c, c.d, splits)
    x, fw = c.x.cuda(), quant.quantize_weight(c.w.cuda())
    y0 = quant.linear_fp8(x, fw, splits=splits)
    assert_bits(y0, c.expected)
    rows = torch.arange(m, device="cuda")
    for j in (0, m - 1):
        y = quant.linear_fp8(fx.poison(x, j, NF_COL, kind), fw, splits=splits)
        assert not bool(torch.isfinite(y[j]).any()), (j, kind)
        assert_bits(y[rows != j], y0[rows != j])


@pytest.mark.parametrize("splits", [1, 2])
def test_inf_weight_scale_stays_in_its_column(cuda, splits):
    m, n, k = 65, 256, 512
    c = fx.int_case(m, n, k)
    fx.check_slabs(c, splits)
    col = 131
    sb = c.sb.clone()
    sb[col] = float("inf")
    y, _ = launch(c.xq.cuda(), c.sa.cuda(), c.wq.cuda(), sb.cuda(), splits, 0, 1)
    cols = torch.arange(n, device="cuda")
    assert not bool(torch.isfinite(y[:, col]).any())
    assert_bits(y[:, cols != col], c.expected.cuda()[:, cols != col])


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_token_through_fp8_moe(cuda, kind):
    """moe.forward with FP8 experts at t = 5: exactly the poisoned token's output row is non-finite
    and the other tokens' rows are bit-identical."""
    t, h, i, e, k = 5, 256, 384, 8, 2
    gen = gx.gen(t, h, i, 23)
    x = (torch.randn(t, h, generator=gen) * 0.5).to(BF).cuda()
    wr = (torch.randn(e, h, generator=gen) * 0.1).to(BF).cuda()
    gu = quant.quantize_experts((torch.randn(e, 2 * i, h, generator=gen) * 0.05).cuda())
    dn = quant.quantize_experts((torch.randn(e, h, i, generator=gen) * 0.05).cuda())
    y0 = moe.forward(x, wr, gu, dn, k)
    assert bool(torch.isfinite(y0).all())
    rows = torch.arange(t, device="cuda")
    for j in (0, t - 1):
        y = moe.forward(fx.poison(x, j, NF_COL, kind), wr, gu, dn, k)
        assert not bool(torch.isfinite(y[j]).any()), (j, kind)
        assert_bits(y[rows != j], y0[rows != j])
