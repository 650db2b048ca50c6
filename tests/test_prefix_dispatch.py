"""Dispatch of the split-context prefill kernel (version 5), on the host: which prefill calls take it by
default, that the in-kernel q-RoPE is then off (the kernel reads a rotated q), and the split plan."""
from distributed_llms_amd import knobs, ops

LLAMA = dict(num_kv_heads=8, group=4)


def _eligible(batch, max_q_len, max_ctx):
    return ops.prefill_split_eligible(batch, LLAMA["num_kv_heads"], max_q_len, max_ctx, LLAMA["group"])


def test_default_cutover_is_the_measured_one():
    assert knobs.Knobs().prefill_split_min_ctx == 4096 and ops.PREFILL_SPLIT == 5


def test_split_kernel_eligibility():
    """Small max_q_len, few sequences, longest context from the knob on; never with the knob at 0, with
    an explicit prefill kernel, without the host knowing the context, or when the plain grid fills the
    device."""
    with knobs.override(prefill_attn=0, prefill_split_min_ctx=4096):
        assert _eligible(1, 20, 8192) and _eligible(1, 1, 4096) and _eligible(8, 64, 4096)
        assert not _eligible(1, 20, 4095) and not _eligible(1, 20, 0) and not _eligible(1, 20, None)
        assert not _eligible(64, 1, 32768)                  # 512 workgroups already
        assert not _eligible(8, 65, 32768)                  # three row tiles x 8 heads x 8 sequences
        # chunks of a chunked prompt (the cutover was measured up to 64 rows; from 384 rows the parent
        # runs the 32x32 kernel, which the split form was never compared with): as before
        assert ops.PF_SPLIT_MAX_Q == 64 and _eligible(1, 64, 8192)
        for b, q in [(1, 65), (1, 128), (1, 384), (1, 512), (2, 256), (4, 128), (1, 4096)]:
            assert not _eligible(b, q, 8192) and not _eligible(b, q, 32768), (b, q)
        assert not ops.prefill_split_eligible(1, 6, 20, 8192, 6)       # a GQA group the 16x16 tiles do not take
    with knobs.override(prefill_split_min_ctx=0):
        assert not _eligible(1, 20, 32768)
    with knobs.override(prefill_split_min_ctx=1024):
        assert _eligible(1, 20, 1024) and not _eligible(1, 20, 1023)
    for v in (3, 4, 7, 9):
        with knobs.override(prefill_attn=v, prefill_split_min_ctx=1024):
            assert not _eligible(1, 20, 8192)


def test_rope_in_attention_off_where_the_split_kernel_is_chosen():
    def rope(max_blocks, batch=1, max_q_len=20, max_ctx=None):      # Llama-3-8B heads
        return ops.prefill_route(batch, 32, 8, 128, max_q_len, max_ctx, max_blocks).rope_in_kernel

    with knobs.override(prefill_attn=0, prefill_fused_rope=True, prefill_split_min_ctx=4096):
        assert rope(256)
        assert not rope(256, 1, 20, 8192)
        assert rope(256, 256, 128, 128)             # the flagship prefill: untouched
        assert rope(256, 1, 20, 4000)
        assert rope(256, 1, 512, 8192)              # a 512-row chunk over 8k: untouched
    with knobs.override(prefill_attn=0, prefill_fused_rope=True, prefill_split_min_ctx=0):
        assert rope(256, 1, 20, 8192)
    with knobs.override(prefill_attn=ops.PREFILL_SPLIT, prefill_fused_rope=True):
        assert not rope(16)                         # forced: every prefill call reads a rotated q


def test_split_plan_fills_the_cus_with_a_floor():
    # one 20-token tail over 8k tokens: v3's grid is 8 workgroups; the plan asks for 32 splits of 8 chunks
    assert ops.prefill_split_plan(1, 8, 20, 8192, 4) == (32, 8)
    # the floor of chunks per split bounds the split count of a short context
    n, sc = ops.prefill_split_plan(1, 8, 1, 1024, 4)
    assert n == 4 and sc == ops.PF_SPLIT_MIN_CHUNKS
    # enough workgroups without splitting
    assert ops.prefill_split_plan(64, 8, 64, 32768, 4)[0] == 1
    # the workspace of an eligible call is bounded: T x Hq x nsplit x (D + 2) floats
    worst = max(b * q * 32 * ops.prefill_split_plan(b, 8, q, 32768, 4)[0] * 130 * 4
                for b in (1, 2, 4, 8, 16) for q in (1, 16, 32, 64) if _eligible(b, q, 32768))
    assert worst <= 256 << 20
