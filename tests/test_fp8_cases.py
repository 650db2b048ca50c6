"""CPU checks of tests/fp8_exact_cases.py: every builder with its preconditions at every shape
the GPU tests of test_fp8_exact.py launch, an emulation of the kernels' contract that passes every
case, and mutants of that emulation -- the errors the cases exist to catch -- each of which must fail
at least one case of its form.  A form that lets its mutant through is not finished."""
import pytest
import torch

import fp8_exact_cases as fx
import gemm_exact_cases as gx
from distributed_llms_amd.ops import quant


def differs(a, b):
    return gx.bits_mismatch(a, b) is not None


# ------------------------------------------------------------------ builders and preconditions
@pytest.mark.parametrize("m,n,k,r,splits", fx.all_int_cases())
def test_int_case_preconditions_and_emulation(m, n, k, r, splits):
    """64 K < 2^24, rounded >= 5 %, ties >= 1 % (asserted by the builder), every scaled slice
    partial unchanged by the slab; the emulation (f32 epilogue, f16 slabs, f32 sum) gives the fp64
    expectation."""
    c = fx.int_case(m, n, k, r)
    worst = fx.check_slabs(c, splits)
    assert r * r * k < 2 ** 24 and c.rounded >= gx.MIN_ROUNDED and c.ties >= gx.MIN_TIES and worst <= gx.SLAB_LIMIT
    assert int(fx.decode(c.xq).abs().max()) == r and int(fx.decode(c.wq).abs().max()) == r
    assert c.sa.unique().numel() == min(m, 5) and c.sb.unique().numel() == 7
    if m * n * k <= 700 * 256 * 1024:
        assert not differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, splits), c.expected)


def test_fp8_slice_rule_matches_the_launcher():
    assert fx.fp8_slices(128, 1) == (1, [(0, 128)])
    assert fx.fp8_slices(384, 2) == (2, [(0, 256), (256, 384)])
    assert fx.fp8_slices(1024, 16)[0] == 8 and fx.fp8_slices(1024, 8)[1][7] == (896, 1024)
    assert fx.fp8_slices(512, 3) == (2, [(0, 256), (256, 512)])
    s, sl = fx.fp8_slices(14336, 7)
    assert s == 7 and sl[6] == (12288, 14336)


@pytest.mark.parametrize("m,n,k", fx.GENERAL_CASES)
def test_general_scale_case(m, n, k):
    """Full-mantissa scales: the expectation is the two-multiply f32 emulation; nearly every output
    is rounded by the bf16 store."""
    c = fx.int_case(m, n, k, 8, "general")
    assert bool((c.sa >= 2.0 ** -6).all()) and bool((c.sa <= 4).all()) and bool((c.sb >= 2.0 ** -6).all())
    assert not differs(fx.emulate(c.xq, c.wq, c.sa, c.sb), c.expected)
    exact = c.acc * c.sa.double()[:, None] * c.sb.double()[None, :]
    assert (c.expected.double() != exact).double().mean().item() > 0.9


@pytest.mark.parametrize("k", [256, 512])
def test_selector_case(k):
    c = fx.selector_case(k, 128, k)
    assert c.rows.unique().numel() == k
    x = fx.decode(c.xq)
    assert bool((x.sum(0) == 1).all()) and bool((x.sum(1) <= 1).all())
    codes = c.wq.unique()
    assert codes.numel() == 253 and not any(b in codes.tolist() for b in (0x7F, 0xFF, 0x80))
    for splits in (1, 2):
        assert not differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, splits), c.expected)


def test_every_finite_e4m3_value_is_exact_in_bf16_and_in_the_slab():
    v = fx.decode(fx.FINITE_CODES.to(torch.uint8))
    assert torch.equal(v.to(torch.bfloat16).double(), v)
    assert torch.equal(fx.through_slab(v.float()).double(), v)
    assert v.abs().max() == 448 and v.abs()[v != 0].min() == 2.0 ** -9


@pytest.mark.parametrize("m,inter,k", sorted({c[:3] for c in fx.SWIGLU_CASES}))
def test_swiglu_case(m, inter, k):
    c = fx.swiglu_case(m, inter, k)
    assert c.gmax <= 256
    gu = fx.decode(c.xq) @ fx.decode(c.wq).t() * 2.0 ** -6
    ref = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
    torch.testing.assert_close(c.ref, ref, rtol=1e-14, atol=0)
    assert gx.swiglu_mismatch(ref.to(torch.bfloat16), c.ref) is None
    assert gx.swiglu_mismatch((ref * (1 + 2.0 ** -7)).to(torch.bfloat16), c.ref) is not None


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("counts,top_k", fx.MOE_ROUTINGS)
def test_moe_case(counts, top_k, gathered):
    rt = fx.routing(counts, top_k)
    n, k = fx.MOE_INT_DIMS[gathered]
    c = fx.moe_case(counts, top_k, n, k, gathered, 0)
    assert k % 128 == 0 and c.sa.shape == (rt.slots,) and c.wscale.shape == (len(counts), n)
    assert not differs(fx.emulate_moe(c, rt, gathered), c.expected)
    inter, k = fx.MOE_SWIGLU_DIMS[gathered]
    s = fx.moe_case(counts, top_k, 2 * inter, k, gathered, 1)
    assert k % 128 == 0 and s.ref.shape == (rt.slots, inter) and bool(torch.isfinite(s.ref).all())


def test_moe_routings_cross_the_row_tile_choice():
    counts = {c for cs, _ in fx.MOE_ROUTINGS for c in cs}
    assert {0, 1, 64, 65, 128, 129, 200}.issubset(counts)


@pytest.mark.parametrize("m,n,k,r", fx.E2E_CASES + [(65, 256, 512, 8)])
def test_e2e_case(m, n, k, r):
    """The reference quantizers return exactly the builder's codes and scales, and every plan's
    slices (and the 2 slices the non-finite test asks for at M = 65) keep their scaled partials in
    the slab."""
    c = fx.e2e_case(m, n, k, r)
    if m == 65:
        fx.check_slabs_of(c.xq, c.wq, c.c, c.d, 2)
        assert not differs(fx.emulate(c.xq, c.wq, c.c, c.d, 2), c.expected)
    q, s = quant.quantize_rows_ref(c.x)
    assert torch.equal(q.view(torch.uint8), c.xq) and torch.equal(s, c.c)
    fw = quant.quantize_weight(c.w)
    assert torch.equal(fw.q.view(torch.uint8), c.wq) and torch.equal(fw.scale, c.d)
    splits = quant.fp8_plan(m, n, k)[0]
    fx.check_slabs_of(c.xq, c.wq, c.c, c.d, splits)
    assert not differs(fx.emulate(c.xq, c.wq, c.c, c.d, splits), c.expected)


def test_e2e_m200_takes_the_two_row_tile_split_plan():
    m, n, k, _ = fx.E2E_CASES[1]
    s, bm = quant.fp8_plan(m, n, k)
    assert m == 200 and bm == 128 and s > 1


@pytest.mark.parametrize("k", fx.QUANT_K)
@pytest.mark.parametrize("m", [1, 3])
def test_quant_rows_case(m, k):
    """Asserted by the builder: scale = c exactly, >= 5 % exact ties, the reference rounds them to
    the even code and agrees with the first-principles quantizer."""
    c = fx.quant_rows_case(m, k)
    assert c.ties >= 0.05 and c.x.shape == (m, k)
    assert bool((fx.decode(c.q).abs().amax(1) == 448).all())


@pytest.mark.parametrize("k,seed", [(256, 0), (256, 1), (8200, 0), (8200, 1), (16392, 0), (136, 1), (2056, 1)])
def test_quant_rows_case_of_the_nonfinite_and_norm_tests(k, seed):
    m = 37 if k in (256, 8200, 16392) else 3
    assert fx.quant_rows_case(m, k, seed).ties >= 0.05


def test_quant_rows_case_holds_every_edge_group():
    c = fx.quant_rows_case(3, 2056)
    v = (c.x.double() / c.scale.double()[:, None])
    mids = (fx.e4m3_grid()[1:] + fx.e4m3_grid()[:-1]) / 2
    assert set(mids.tolist()).issubset(set(v.abs().unique().tolist()))              # every midpoint, 17, 19, 8.5 ...
    for edge in (2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 446.0):
        assert bool((v.abs() == edge).any()), edge
    assert bool(((v == 0) & torch.signbit(v)).any()) and bool(((v == 0) & ~torch.signbit(v)).any())
    q = fx.decode(c.q)
    assert bool((q[v.abs() == 2.0 ** -10] == 0).all()) and bool((q[v.abs() == 2.0 ** -11] == 0).all())
    assert bool((q[v == 3 * 2.0 ** -10] == 2.0 ** -8).all()) and bool((q[v == 17] == 16).all())
    assert bool((q[v == 19] == 20).all()) and bool((q[v == 446] == 448).all())


# ------------------------------------------------------------------ mutants
def test_mutant_sa_one_row_off():
    c = fx.int_case(65, 256, 512)
    assert differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, 1, "sa_shift"), c.expected)


def test_mutant_sb_one_column_off():
    c = fx.int_case(65, 256, 512)
    assert differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, 1, "sb_shift"), c.expected)


@pytest.mark.parametrize("counts,top_k", fx.MOE_ROUTINGS)
def test_mutant_sa_by_token_instead_of_slot(counts, top_k):
    rt = fx.routing(counts, top_k)
    n, k = fx.MOE_INT_DIMS[True]
    c = fx.moe_case(counts, top_k, n, k, True, 0)
    assert differs(fx.emulate_moe(c, rt, True, "sa_by_token"), c.expected)


@pytest.mark.parametrize("k", [256, 512])
def test_mutant_chunks_swapped(k):
    c = fx.selector_case(k, 128, k)
    assert differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, 1, "swap_chunks"), c.expected)
    i = fx.int_case(65, 256, 512)                 # the integer form sees it as well
    assert differs(fx.emulate(i.xq, i.wq, i.sa, i.sb, 1, "swap_chunks"), i.expected)


@pytest.mark.parametrize("k,splits", [(384, 2), (1024, 8), (512, 3)])
def test_mutant_last_k_tile_of_a_slice_dropped(k, splits):
    c = fx.int_case(65, 128 if k != 512 else 256, k)
    assert differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, splits, "drop_tile"), c.expected)


def test_mutant_truncating_bf16_store():
    c = fx.int_case(65, 256, 512)
    assert differs(fx.emulate(c.xq, c.wq, c.sa, c.sb, 1, "trunc_store"), c.expected)
    g = fx.int_case(129, 384, 256, 8, "general")
    assert differs(fx.emulate(g.xq, g.wq, g.sa, g.sb, 1, "trunc_store"), g.expected)


@pytest.mark.parametrize("k", [8, 2056])
def test_mutant_truncating_e4m3_conversion(k):
    c = fx.quant_rows_case(3, k)
    q, s = fx.quantize_emulated(c.x)
    assert torch.equal(q, c.q) and torch.equal(s, c.scale)
    qt, _ = fx.quantize_emulated(c.x, rounding="trunc")
    assert not torch.equal(qt, c.q)


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("j", [0, 36])
def test_nonfinite_contract_and_the_clamping_mutant(j, kind):
    """quantize_rows_ref and the emulation keep the contract; fmaxf-style clamping (a NaN never
    reaches amax and converts as -448) is caught for the NaN."""
    x = fx.quant_rows_case(37, 256).x
    q0, s0 = quant.quantize_rows_ref(x)
    xp = fx.poison(x, j, 70, kind)
    q, s = quant.quantize_rows_ref(xp)
    assert fx.nonfinite_contract(s, q, s0, q0, j, kind) is None
    q, s = fx.quantize_emulated(xp)
    assert fx.nonfinite_contract(s, q, s0, q0, j, kind) is None
    q, s = fx.quantize_emulated(xp, nan="clamp")
    if kind == "nan":
        assert "NaN" in fx.nonfinite_contract(s, q, s0, q0, j, kind)
        assert q[j, 70].item() == 0xFE                                    # -448: a plausible finite code


def test_nonfinite_scales_make_the_reference_product_nonfinite():
    x = fx.e2e_case(5, 256, 512).x
    w = quant.quantize_weight(fx.e2e_case(5, 256, 512).w)
    y0 = quant.linear_ref(x, w)
    for kind in ("nan", "inf"):
        y = quant.linear_ref(fx.poison(x, 2, 70, kind), w)
        assert not bool(torch.isfinite(y[2]).any())
        keep = torch.arange(5) != 2
        assert torch.equal(y[keep], y0[keep])
