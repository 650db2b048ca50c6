"""CPU checks of tests/gemm_exact_cases.py: the input builders, the fp64 references and the
preconditions the GPU tests of test_gemm_exact.py / test_moe_exact.py rest on (exactness bounds,
rounded and tie shares, slab identity), against torch's own fp64 matmul."""
import pytest
import torch

import gemm_exact_cases as gx
import moe_exact_cases as mx


@pytest.mark.parametrize("m,n,k,r,splits", gx.all_int_cases())
def test_int_case_preconditions(m, n, k, r, splits):
    """Every integer case a GPU test launches: K r^2 < 2^24, rounded >= 5 %, ties >= 1 % (asserted
    by the builder), every slice partial <= 2048, and an f32 matmul of the same operands -- exact in
    any order under these bounds -- rounds to the same bf16 as the fp64 one."""
    c = gx.int_case(m, n, k, r)
    gx.check_slabs(c, splits)
    assert k * r * r < 2 ** 24 and c.rounded >= 0.05 and c.ties >= 0.01
    if m * n * k <= 300 * 1024 * 4096:
        y32 = c.x.float() @ c.w.float().t()
        assert torch.equal(y32.to(torch.bfloat16), c.expected)
        assert torch.equal(y32.double(), c.x.double() @ c.w.double().t())


def test_slice_rule_matches_the_launchers():
    assert gx.slice_rule(64, 2) == (1, 1)
    assert gx.slice_rule(128, 16) == (2, 1)
    assert gx.slice_rule(192, 2) == (2, 2)
    assert gx.slice_rule(512, 5) == (4, 2)
    assert gx.slice_rule(14336, 16) == (16, 14)


def test_bf16_shares_counts_ties_and_rounded():
    # 257 = 256 + half a bf16 step (2): a tie; 258 is representable; 1001 is rounded, not a tie
    # (step 4 in [512, 1024): 1001 = 1000 + 1); 1002 is a tie
    y = torch.tensor([[257.0, 258.0, 1001.0, 1002.0, -259.0, 3.0, 0.0, 100.0]], dtype=torch.float64)
    rounded, ties = gx.bf16_shares(y)
    assert rounded == 4 / 8 and ties == 3 / 8
    assert torch.tensor(257.0).to(torch.bfloat16).item() == 256.0      # ties to even
    assert torch.tensor(259.0).to(torch.bfloat16).item() == 260.0


def test_slab_limit_is_the_f16_integer_range():
    v = torch.arange(-2048, 2049, dtype=torch.float32).to(torch.bfloat16).float()
    i = torch.arange(-2048, 2049, dtype=torch.float32)
    assert bool(((i * 2.0 ** -6).half().float() * 64 == i).all())
    assert not bool(((torch.tensor(2049.0) * 2.0 ** -6).half().float() * 64 == 2049.0))
    assert bool(gx.survives_slab(v.to(torch.bfloat16)).all())


@pytest.mark.parametrize("m,n,k", [(512, 256, 64), (512, 256, 192), (512, 256, 512), (256, 256, 256)])
def test_selector_case(m, n, k):
    c = gx.selector_case(m, n, k)
    assert c.rows.unique().numel() == k                       # each k selected by exactly one row
    assert bool((c.x.float().sum(0) == 1).all()) and bool((c.x.float().sum(1) <= 1).all())
    y = (c.x.double() @ c.w.double().t()).to(torch.bfloat16)
    assert torch.equal(y.view(torch.int16)[c.rows], c.expected.view(torch.int16)[c.rows])
    assert torch.equal(y, c.expected)
    w = c.w.float()
    assert bool((w < 0).any()) and bool((w > 0).any()) and w.abs().max() < 2 ** 9 and w.abs().min() >= 2 ** -8
    assert bool(gx.survives_slab(c.w).all())


@pytest.mark.parametrize("m,inter,k", sorted(set(gx.SWIGLU_WIDE + gx.SWIGLU_SQ +
                                                 gx.SWIGLU_PF + [c[1:] for c in gx.SWIGLU_PP] +
                                                 [c[1:] for c in gx.SWIGLU_DISPATCH_CASES] +
                                                 [(257, 256, 128), (4100, 256, 128)])))
def test_swiglu_case(m, inter, k):
    c = gx.swiglu_case(m, inter, k)
    assert c.gmax <= 256
    gu = c.x.double() @ c.w.double().t()
    # gate and up are exact in bf16 (gemm_pp's two-phase epilogue) and in the f16 x 2^-6 slabs
    assert torch.equal(gu.to(torch.bfloat16).double(), gu)
    assert torch.equal((gu.float() * 2.0 ** -6).half().double() * 64, gu)
    ref = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
    torch.testing.assert_close(c.ref, ref, rtol=1e-14, atol=0)
    assert gx.swiglu_mismatch(ref.to(torch.bfloat16), c.ref) is None          # RNE store passes
    assert gx.swiglu_mismatch((ref * (1 + 2.0 ** -7)).to(torch.bfloat16), c.ref) is not None


def test_bits_mismatch_reports_first_position():
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4).to(torch.bfloat16)
    b = a.clone()
    assert gx.bits_mismatch(a, b) is None
    b[1, 2] = 100
    b[2, 0] = 7
    msg = gx.bits_mismatch(b, a)
    assert msg.startswith("2 of 12") and "(m=1, n=2)" in msg and "100.0" in msg and "6.0" in msg


@pytest.mark.parametrize("counts,top_k", mx.ROUTINGS)
def test_moe_routing_builder(counts, top_k):
    r = mx.routing(counts, top_k)
    e = len(counts)
    assert r.offsets.tolist() == [sum(counts[:i]) for i in range(e + 1)]
    assert torch.equal(torch.bincount(r.gather.long(), minlength=r.t), torch.full((r.t,), top_k))
    assert torch.equal(r.gather[r.inv.long()].reshape(r.t, top_k), torch.arange(r.t).repeat_interleave(top_k)
                       .reshape(r.t, top_k).int())
    for i in range(e):
        assert bool((r.slot_expert[r.offsets[i]:r.offsets[i + 1]] == i).all())


@pytest.mark.parametrize("counts,top_k", mx.ROUTINGS)
@pytest.mark.parametrize("dims", [0, 1])
def test_moe_int_case(counts, top_k, dims):
    r = mx.routing(counts, top_k)
    for gathered in (True, False):
        n, k = mx.INT_DIMS[dims][gathered]
        c = mx.moe_int_case(counts, top_k, n, k, gathered)
        xs = c.x[r.gather.long()] if gathered else c.x
        pick = torch.arange(0, r.slots, max(1, r.slots // 37))          # a slot-by-slot check of a sample
        y = torch.einsum("sk,snk->sn", xs.double()[pick], c.w.double()[r.slot_expert.long()[pick]])
        assert torch.equal(y.to(torch.bfloat16), c.expected[pick])
        assert c.rounded >= 0.05 and c.ties >= 0.01


@pytest.mark.parametrize("counts,top_k", mx.ROUTINGS)
@pytest.mark.parametrize("dims", [0, 1])
def test_moe_swiglu_case(counts, top_k, dims):
    """Every gate / up sum of every slot is an integer <= 256 x 2^-6 (asserted by the builder), exact
    in bf16 and in f16 x 2^-6; a sample of slots is recomputed row by row."""
    r = mx.routing(counts, top_k)
    for gathered in (True, False):
        inter, k = mx.SWIGLU_DIMS[dims][gathered]
        c = mx.moe_swiglu_case(counts, top_k, inter, k, gathered)
        xs = c.x[r.gather.long()] if gathered else c.x
        pick = torch.arange(0, r.slots, max(1, r.slots // 37))
        gu = torch.einsum("sk,snk->sn", xs.double()[pick], c.w.double()[r.slot_expert.long()[pick]])
        assert bool((gu.abs() * 64 <= 256).all()) and torch.equal(gu.to(torch.bfloat16).double(), gu)
        ref = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        torch.testing.assert_close(c.ref[pick], ref, rtol=1e-14, atol=0)


def test_bits_mismatch_tolerates_matching_nans():
    a = torch.tensor([[1.0, float("nan")]], dtype=torch.bfloat16)
    assert gx.bits_mismatch(a, a.clone()) is None
    assert "(m=0, n=0)" in gx.bits_mismatch(a, torch.tensor([[2.0, float("nan")]], dtype=torch.bfloat16))


def test_moe_combine_case_is_exact_in_f32():
    for t, top_k in mx.COMBINE_CASES:
        c = mx.combine_case(t, top_k, 264)
        acc = torch.zeros(t, 264)
        for j in range(top_k):
            acc += c.topk_w[:, j:j + 1] * c.ys[c.inv.long().reshape(t, top_k)[:, j]].float()
        assert torch.equal(acc.double(), c.exact)


@pytest.mark.parametrize("e", [4, 8, 16])
@pytest.mark.parametrize("t", [1, 5, 300])
def test_route_case_margins(e, t):
    c = mx.route_case(t, e, 2)
    lg = c.logits.float()
    top = lg.topk(3, dim=-1).values
    assert bool((top[:, 0] - top[:, 1] >= 1).all()) and bool((top[:, 1] - top[:, 2] >= 4).all())
    assert not bool((c.ids == c.idle).any())
    # the fused router's operands reproduce these logits exactly
    assert torch.equal((c.rx.double() @ c.rw.double().t()).to(torch.bfloat16), c.logits)
