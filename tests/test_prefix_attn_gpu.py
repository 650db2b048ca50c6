"""The split-context prefill kernel (version 5): a few query rows over a long cached context, the shape
a prefix-cache hit produces.  Position-exact cases with the builders, the poison and the one assertion
of test_attention_exact.py at pairs that put split boundaries on and off block edges, leave splits
empty, have no cached context, a partial last block and rows past a sequence's q_len; then the
partial workspace, run-to-run bits and random inputs against ops.reference."""
import math

import pytest
import torch

import test_attention_exact as ax
from distributed_llms_amd import knobs, ops
from distributed_llms_amd.ops import reference as ref

# (ctx, q_len): one packed batch.  132 chunks at most (4200 keys), so 200 forced splits leave 68 empty
PAIRS = ((300, 1), (65, 1), (2049, 3), (2048, 4), (2080, 5), (1000, 33), (37, 37), (4200, 17))
HEADS = [(32, 8, 128), (8, 4, 128), (32, 2, 128), (12, 12, 64)]        # G = 4, 2, 16, 1
NSPLIT = [1, 2, 7, 200, None]                                           # None: ops.prefill_split_plan
V5 = ops.PREFILL_SPLIT


# ------------------------------------------------------------------ CPU self-checks
@pytest.mark.parametrize("form", ax.FORMS)
@pytest.mark.parametrize("hq,hkv,d", HEADS)
def test_cpu_reference_passes_split_cases(hq, hkv, d, form):
    c = ax.prefill_case(form, hq, hkv, d, PAIRS)
    got = ref.paged_attention_prefill(c.q.float(), c.k.float(), c.v.float(), c.bt, c.cu, c.sl, 1 / math.sqrt(d))
    ax.assert_exact(got, c.expect)


@pytest.mark.parametrize("mutant", list(ax.PREFILL_MUTANTS))
@pytest.mark.parametrize("form", ax.FORMS)
def test_prefill_mutants_are_rejected_at_the_split_pairs(form, mutant):
    c = ax.prefill_case(form, 8, 4, 128, PAIRS)
    cu = c.cu.tolist()
    for i, (n, ql) in enumerate(c.pairs):
        q, want = c.q[cu[i]:cu[i + 1]], c.expect[cu[i]:cu[i + 1]]
        with pytest.raises(AssertionError):
            ax.assert_exact(ax.PREFILL_MUTANTS[mutant](c, q, c.ks[i], c.vs[i], n - ql), want)


def test_split_plan_covers_the_context():
    """The planned splits cover every chunk, keep the floor of chunks per split and stop at one split
    where the plain grid already fills the device."""
    for b, hkv, mq, ctx, g in [(1, 8, 20, 8192, 4), (8, 8, 5, 4096, 4), (1, 2, 1, 300, 16), (64, 8, 64, 32768, 4),
                               (1, 8, 17, 4200, 4), (1, 12, 37, 37, 1)]:
        n, sc = ops.prefill_split_plan(b, hkv, mq, ctx, g)
        chunks = -(-ctx // 32)
        assert n >= 1 and n * sc >= chunks and (n - 1) * sc < chunks
        assert n == 1 or sc >= ops.PF_SPLIT_MIN_CHUNKS
    assert ops.prefill_split_plan(1, 8, 20, 8192, 4)[0] > 1
    assert ops.prefill_split_plan(256, 8, 64, 8192, 4)[0] == 1


# ------------------------------------------------------------------ on the GPU
def _run(c, nsplit, **kw):
    q, k, v, bt, cu, sl = ax._dev(c, "q", "k", "v", "bt", "cu", "sl")
    return ops.paged_attention_prefill(q, k, v, bt, cu, sl, 1 / math.sqrt(c.d), max_q_len=c.max_q, version=V5,
                                       max_ctx=max(c.lens), nsplit=nsplit, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("nsplit", NSPLIT)
@pytest.mark.parametrize("form", ax.FORMS)
@pytest.mark.parametrize("heads", HEADS, ids=lambda x: str(x).replace(", ", "-"))
def test_prefill_split_exact(cuda, heads, form, nsplit):
    c = ax.prefill_case(form, *heads, PAIRS)
    ax.assert_exact(_run(c, nsplit), c.expect)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ax.FORMS)
def test_prefill_split_one_tile_per_wave_exact(cuda, form):
    """max_q_len small enough for one tile per wave (the kernel's other instantiation), alone and as a
    batch, also through the knob that forces the kernel."""
    pairs = tuple(p for p in PAIRS if p[1] <= 5)
    for heads in HEADS:
        c = ax.prefill_case(form, *heads, pairs)
        for nsplit in (1, 7, None):
            ax.assert_exact(_run(c, nsplit), c.expect)
    c = ax.prefill_case(form, 32, 8, 128, pairs)
    q, k, v, bt, cu, sl = ax._dev(c, "q", "k", "v", "bt", "cu", "sl")
    with knobs.override(prefill_attn=V5):
        assert not ops.prefill_route(len(pairs), 32, 8, 128, c.max_q, None, bt.shape[1]).rope_in_kernel
        ax.assert_exact(ops.paged_attention_prefill(q, k, v, bt, cu, sl, 1 / math.sqrt(c.d), max_q_len=c.max_q),
                        c.expect)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ax.FORMS)
def test_prefill_split_nan_workspace_and_same_bits(cuda, form):
    """An oversized, NaN-filled partial workspace: every partial the reduce reads was written, empty
    splits included; and two runs give the same bits."""
    c = ax.prefill_case(form, 32, 8, 128, PAIRS)
    t = c.q.shape[0]
    for nsplit in (7, 200):
        def ws():
            return (torch.full((t * c.hq * nsplit * c.d + 7,), float("nan"), device="cuda"),
                    torch.full((t * c.hq * nsplit * 2 + 7,), float("nan"), device="cuda"))
        a = _run(c, nsplit, workspace=ws())
        b = _run(c, nsplit, workspace=ws())
        assert not a.isnan().any()
        ax.assert_exact(a, c.expect)
        assert torch.equal(a, b)
    assert torch.equal(_run(c, None), _run(c, None))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ax.FORMS)
def test_prefill_split_host_context_below_a_sequence(cuda, form):
    """A plan made for a shorter context than a sequence on the device has (max_ctx 1024 against 4200
    keys): the last split runs to the causal bound, no key is dropped."""
    c = ax.prefill_case(form, 32, 8, 128, PAIRS)
    q, k, v, bt, cu, sl = ax._dev(c, "q", "k", "v", "bt", "cu", "sl")
    for nsplit in (None, 1, 3):
        out = ops.paged_attention_prefill(q, k, v, bt, cu, sl, 1 / math.sqrt(c.d), max_q_len=c.max_q, version=V5,
                                          max_ctx=1024, nsplit=nsplit)
        ax.assert_exact(out, c.expect)


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv,d", HEADS)
def test_prefill_split_random_against_reference(cuda, hq, hkv, d):
    """Random bf16 inputs at the tolerance of test_kernels_gpu.py's prefill-against-reference tests."""
    c = ax.prefill_case("random", hq, hkv, d, PAIRS)
    q, k, v, bt, cu, sl = ax._dev(c, "q", "k", "v", "bt", "cu", "sl")
    scale = 1 / math.sqrt(d)
    expect = ref.paged_attention_prefill(q.float(), k.float(), v.float(), bt, cu, sl, scale)
    for nsplit in (None, 7):
        torch.testing.assert_close(_run(c, nsplit).float(), expect, atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
def test_prefill_split_chosen_by_default_from_the_knob(cuda):
    """With the cutover knob set, the default dispatch takes the split kernel for a short tail over a
    long context (same bits as forcing it) and not for a batch that fills the device."""
    c = ax.prefill_case("needle", 32, 8, 128, PAIRS)
    q, k, v, bt, cu, sl = ax._dev(c, "q", "k", "v", "bt", "cu", "sl")
    scale = 1 / math.sqrt(c.d)
    with knobs.override(prefill_split_min_ctx=1024):
        assert ops.prefill_split_eligible(len(PAIRS), c.hkv, c.max_q, max(c.lens), c.hq // c.hkv)
        auto = ops.paged_attention_prefill(q, k, v, bt, cu, sl, scale, max_q_len=c.max_q, max_ctx=max(c.lens))
    assert torch.equal(auto, _run(c, None))
    ax.assert_exact(auto, c.expect)


# ------------------------------------------------------------------ the route's two demotions
def _small(d, width=None):
    """Seeded: B = 2, query lengths (5, 33) over contexts (5, 70), hq, hkv = 4, 2; ``width``: block-table
    columns to pad to (the padding is never read)."""
    c = ax.prefill_case("random", 4, 2, d, ((5, 5), (70, 33)))
    q, k, v, bt, cu, sl = ax._dev(c, "q", "k", "v", "bt", "cu", "sl")
    if width is not None:
        bt = torch.nn.functional.pad(bt, (0, width - bt.shape[1])).contiguous()
    return lambda version: ops.paged_attention_prefill(q, k, v, bt, cu, sl, 1 / math.sqrt(d), max_q_len=c.max_q,
                                                       version=version)


@pytest.mark.gpu
def test_w32_version_at_head_dim_64_runs_version_4(cuda):
    run = _small(64)
    assert torch.equal(run(9), run(4))


@pytest.mark.gpu
def test_lds_version_behind_a_wide_block_table_runs_version_3(cuda):
    run = _small(128, ops.PF_MAX_CHUNKS + 1)
    assert torch.equal(run(4), run(3))
