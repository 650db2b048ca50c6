"""The grouped MoE kernels driven directly, with routings built by hand and operands whose result
is known exactly (input forms and bounds: tests/test_gemm_exact.py; builders:
tests/moe_exact_cases.py, checked on the CPU by tests/test_exact_cases.py).

  grouped GEMMs   moe_wide_gemm (deep and 3-slot ring), moe_grouped_gemm (variants 0 .. 6) and
                  gemm_pp_moe get counts / offsets / gather written by the test.  Mode 0: integer x
                  and per-expert integer weights (all different, so a slot multiplied by a
                  neighbour's weights is wrong everywhere): y[slot] must equal
                  bf16(x[gather[slot]] @ w[e]^T) bit for bit (K r^2 = 512 x 64 < 2^24).  Mode 1
                  (SwiGLU): ternary x 2^-6 operands at rtol 2^-8 + 2^-12, atol 1e-30 (part E of
                  test_gemm_exact.py).  y sits between sentinel rows; with the counts / offsets
                  pointers advanced to a sub-range of the experts (what expert parallelism passes),
                  the slots of the other experts must stay sentinels as well.
  moe_combine     integer ys (|y| <= 2000, 11 bits) and power-of-two weights 1 .. 1/8: every product
                  and the sum of top_k of them is exact in f32, so the output is the fp64 sum rounded
                  to bf16, bit for bit.
  routing         logits whose top-k is separated by >= 1 between chosen experts and >= 4 to the
                  rest, all exact in bf16 (for the fused router: x and unit-vector router weights
                  whose products are these logits exactly), so no accumulation order can flip a
                  choice.  ids, counts, offsets, sorted_tok and inv are then fully determined up to
                  the order inside a segment; the top-k weights are an f32 softmax over <= 16 values
                  renormalised over 2: rtol 1e-5 against the fp32 reference.
  expert parallel moe.forward(expert_offset=o) over halves and quarters of the experts.  Tokens with
                  no local expert give exact zeros.  The float sum of the parts against the full
                  forward: each part is bf16(a_i) of the f32 partial sums a_i, the full output
                  bf16(sum a_i).  All operands here are >= 0, so every a_i >= 0 and nothing cancels:
                  |sum of parts - full| <= sum_i ulp(a_i) / 2 + ulp(full) / 2, and with at most two
                  non-zero parts (top_k = 2) the smaller one's half ulp and the full output's are
                  each <= 2^-8 of the sum.  Hence rtol 2^-7 on the sum plus atol of half a bf16 ulp
                  of the largest part.  (With mixed signs two parts may cancel and leave both of
                  their rounding errors beside a small sum; the bound is not derivable there.)
"""
import pytest
import torch

import gemm_exact_cases as gx
import moe_exact_cases as mx
from distributed_llms_amd import _ext
from distributed_llms_amd.ops import moe
from distributed_llms_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
G = gx.GUARD_ROWS
assert_bits, sentinel_out, assert_untouched = gx.assert_bits, gx.sentinel_out, gx.assert_untouched

KERNELS = [("wide", 0), ("wide", 4)] + [("grouped", v) for v in range(7)] + [("pp", 0)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def grouped_launch(kern, arg, y, x, gather, w, counts, offsets, e, n, k, xrows, slots, mode):
    kk = _ext.kernels()
    gp = gather.data_ptr() if gather is not None else 0
    if kern == "wide":
        kk.moe_wide_gemm(y.data_ptr(), x.data_ptr(), gp, w.data_ptr(), counts, offsets, e, n, k, mode | arg, _stream())
    elif kern == "grouped":
        kk.moe_grouped_gemm(y.data_ptr(), x.data_ptr(), gp, w.data_ptr(), counts, offsets, e, n, k, mode,
                            (1, 16, 64)[arg % 3], arg, _stream())
    else:
        kk.gemm_pp_moe(y.data_ptr(), x.data_ptr(), gp, w.data_ptr(), counts, offsets, e, n, k, xrows, slots, mode,
                       _stream())


@pytest.mark.parametrize("kern,arg", KERNELS)
@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("dims", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("counts,top_k", mx.ROUTINGS)
def test_grouped_gemm_slot_expert_mapping(cuda, counts, top_k, mode, dims, gathered, kern, arg):
    """Every slot is multiplied by its own expert's weights and by the row gather names (first
    projection) or its own row (second projection, gather = 0); empty experts, one expert owning
    everything, and row tiles that end inside a segment; nothing outside the slot rows is written."""
    rt = mx.routing(counts, top_k)
    e = len(counts)
    if mode == 0:
        n, k = mx.INT_DIMS[dims][gathered]
        c = mx.moe_int_case(counts, top_k, n, k, gathered)
        cols = n
    else:
        inter, k = mx.SWIGLU_DIMS[dims][gathered]
        c = mx.moe_swiglu_case(counts, top_k, inter, k, gathered)
        n, cols = 2 * inter, inter
    x, w = c.x.cuda(), c.w.cuda()
    cnt, off = rt.counts.cuda(), rt.offsets.cuda()
    gather = rt.gather.cuda() if gathered else None
    buf, y = sentinel_out(rt.slots, cols)
    grouped_launch(kern, arg, y, x, gather, w, cnt.data_ptr(), off.data_ptr(), e, n, k, x.shape[0], rt.slots, mode)
    if mode == 0:
        assert_bits(y, c.expected)
    else:
        msg = gx.swiglu_mismatch(y, c.ref)
        assert msg is None, msg
    assert_untouched(buf[:G], "rows before slot 0")
    assert_untouched(buf[G + rt.slots:], "rows past the last slot")


@pytest.mark.parametrize("kern,arg", [("wide", 0), ("grouped", 0), ("grouped", 3), ("pp", 0)])
@pytest.mark.parametrize("lo,hi", [(2, 6), (4, 8), (0, 2)])
@pytest.mark.parametrize("counts,top_k", [mx.ROUTINGS[0], mx.ROUTINGS[2]])
def test_grouped_gemm_local_expert_range(cuda, counts, top_k, lo, hi, kern, arg):
    """Expert parallelism: counts / offsets advanced to experts [lo, hi) and only their weights
    passed.  Their slots hold the exact products; every other slot stays untouched."""
    rt = mx.routing(counts, top_k)
    n, k = 512, 256
    c = mx.moe_int_case(counts, top_k, n, k, True)
    x, w = c.x.cuda(), c.w[lo:hi].contiguous().cuda()
    cnt, off, gather = rt.counts.cuda(), rt.offsets.cuda(), rt.gather.cuda()
    buf, y = sentinel_out(rt.slots, n)
    grouped_launch(kern, arg, y, x, gather, w, cnt.data_ptr() + 4 * lo, off.data_ptr() + 4 * lo, hi - lo, n, k,
                   x.shape[0], rt.slots, 0)
    a, b = rt.offsets[lo].item(), rt.offsets[hi].item()
    assert_bits(y[a:b], c.expected[a:b])
    assert_untouched(buf[:G + a], "slots of the experts below the local range")
    assert_untouched(buf[G + b:], "slots of the experts above the local range")


@pytest.mark.parametrize("h", [264, 4096])
@pytest.mark.parametrize("t,top_k", mx.COMBINE_CASES)
def test_moe_combine_exact(cuda, t, top_k, h):
    c = mx.combine_case(t, top_k, h)
    ys, tw, inv = c.ys.cuda(), c.topk_w.cuda(), c.inv.cuda()
    buf, out = sentinel_out(t, h)
    _ext.kernels().moe_combine(out.data_ptr(), ys.data_ptr(), tw.data_ptr(), inv.data_ptr(), t, h, top_k, _stream())
    assert_bits(out, c.exact.to(BF))
    assert_untouched(buf[:G], "rows before the output")
    assert_untouched(buf[G + t:], "rows past the output")


def check_slot_layout(c, t, e, k, topk_w, topk_ids, counts, offsets, sorted_tok, inv):
    topk_w, topk_ids, counts, offsets, sorted_tok, inv = (v.cpu() for v in (topk_w, topk_ids, counts, offsets,
                                                                          sorted_tok, inv))
    rw, rid = ref.moe_route(c.logits.float(), k)
    so, ro = topk_ids.long().argsort(1), rid.long().argsort(1)
    assert torch.equal(topk_ids.long().gather(1, so), rid.long().gather(1, ro))          # sets per token
    assert torch.equal(rid.long().gather(1, ro), c.ids.long().sort(1).values)
    torch.testing.assert_close(topk_w.gather(1, so), rw.gather(1, ro), rtol=1e-5, atol=0)
    assert torch.equal(counts.long(), torch.bincount(topk_ids.reshape(-1).long(), minlength=e))
    assert counts[c.idle].item() == 0
    assert offsets[0].item() == 0 and torch.equal(offsets[1:].long(), counts.long().cumsum(0))
    assert offsets[e].item() == t * k
    slot_expert = torch.repeat_interleave(torch.arange(e), counts.long())
    # the segment of expert e holds exactly the tokens that chose e
    have = (sorted_tok.long() * e + slot_expert).sort().values
    want = (torch.arange(t).unsqueeze(1) * e + topk_ids.long()).reshape(-1).sort().values
    assert torch.equal(have, want)
    flat = inv.reshape(-1).long()
    assert torch.equal(flat.sort().values, torch.arange(t * k))
    assert torch.equal(sorted_tok.long()[flat].reshape(t, k), torch.arange(t).unsqueeze(1).expand(t, k))
    assert torch.equal(slot_expert[flat].reshape(t, k), topk_ids.long())


def route_outputs(t, e, k):
    dev = "cuda"
    return (torch.empty(t, k, dtype=torch.float32, device=dev), torch.empty(t, k, dtype=torch.int32, device=dev),
            torch.empty(e, dtype=torch.int32, device=dev), torch.empty(e + 1, dtype=torch.int32, device=dev),
            torch.full((t * k,), -1, dtype=torch.int32, device=dev), torch.full((t * k,), -1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("t", [1, 5, 64, 300, 4096])
@pytest.mark.parametrize("e", [4, 8, 16])
def test_moe_route_slot_layout(cuda, e, t):
    k = 2
    c = mx.route_case(t, e, k)
    outs = route_outputs(t, e, k)
    logits = c.logits.cuda()
    _ext.kernels().moe_route(logits.data_ptr(), t, e, k, *(o.data_ptr() for o in outs), _stream())
    check_slot_layout(c, t, e, k, *outs)


@pytest.mark.parametrize("t", [1, 5, 64, 300, 4096])
@pytest.mark.parametrize("e", [8, 16])
def test_moe_router_route_slot_layout(cuda, e, t):
    """The fused router (GEMV + top-k, then the scatter kernel) on operands whose products are the
    same logits exactly.  E = 4 is not a case here: the launcher accepts 8 or 16 experts only
    (moe.hip, moe_router_route); moe_route above covers E = 4."""
    k = 2
    c = mx.route_case(t, e, k)
    outs = route_outputs(t, e, k)
    x, w = c.rx.cuda(), c.rw.cuda()
    _ext.kernels().moe_router_route(x.data_ptr(), w.data_ptr(), t, x.shape[1], e, k, *(o.data_ptr() for o in outs),
                                    _stream())
    check_slot_layout(c, t, e, k, *outs)


def half_ulp_bf16(v):
    a = v.abs()
    return torch.where(a > 0, torch.pow(2.0, torch.floor(torch.log2(a.clamp(min=1e-30))) - 8), torch.zeros_like(a))


@pytest.mark.parametrize("parts", [2, 4])
@pytest.mark.parametrize("t", [64, 300])
def test_expert_parallel_parts_sum_to_full(cuda, t, parts):
    """moe.forward(expert_offset=o) at a decode-sized and a prefill-sized T, experts in halves and
    quarters (bound: module docstring; operands >= 0 so that it is derivable)."""
    e, k, h, i = 8, 2, 256, 256
    gen = gx.gen(t, parts, 21)
    logits = torch.randint(0, 9, (t, e), generator=gen).float() * 0.25            # [0, 2]
    ids = torch.rand(t, e, generator=gen).argsort(1)[:, :k]
    ids[::7] = torch.tensor([0, 1])                       # some tokens certainly miss the upper parts
    for j in range(k):
        logits[torch.arange(t), ids[:, j]] = 8.0 - j
    x = (torch.randn(t, h, generator=gen).abs() * 0.5)
    x[:, :e] = logits
    wr = torch.zeros(e, h)
    wr[torch.arange(e), torch.arange(e)] = 1.0
    wgu = torch.randn(e, 2 * i, h, generator=gen).abs() * 0.05
    wd = torch.randn(e, h, i, generator=gen).abs() * 0.05
    x, wr, wgu, wd = (v.to(BF).cuda() for v in (x, wr, wgu, wd))
    full = moe.forward(x, wr, wgu, wd, k).float()
    assert bool((full > 0).all())
    n = e // parts
    outs = []
    for p in range(parts):
        o = p * n
        out = moe.forward(x, wr, wgu[o:o + n].contiguous(), wd[o:o + n].contiguous(), k, expert_offset=o).float()
        away = ~((ids >= o) & (ids < o + n)).any(1)
        assert bool(away.any())
        assert bool((out[away.cuda()] == 0).all()), "a token with no local expert must give exact zeros"
        assert bool((out[~away.cuda()] > 0).all())
        outs.append(out)
    parts_t = torch.stack(outs)
    total = parts_t.sum(0)
    err = (total - full).abs()
    bound = 2.0 ** -7 * total.abs() + half_ulp_bf16(parts_t.abs().max(0).values)
    assert bool((err <= bound).all()), f"worst err / bound {(err / bound).max().item()}"
