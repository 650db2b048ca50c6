"""The per-token kernels of csrc/kernels/norm_elementwise.hip (and the fused decode append of
attention.hip) against fp64 expectations on the inputs of tests/pertoken_cases.py: bit for bit where the
f32 evaluation is exact, within half a bf16 ulp + 2^-12 elsewhere, guard rows and sentinels around every
output, inputs unchanged (gfx950 only).  The rules, and why they reject the mistakes these kernels are
prone to, are in pertoken_cases.py and test_pertoken_cases.py.

What launches what:
  rms_norm_kernel<1> / <2> / <4> / <8>   test_rms_norm / test_fused_add_rms_norm at hidden 8, 136, 2048 /
                                         2056, 4096 / 4104, 8192 / 8200, 16384: each instance with a full
                                         and with a nearly empty last chunk, with and without a residual
  rope_cache_kernel                      test_rope_cache_append: cos_sin None, block size 16 and 32 (krow /
                                         vofs both branches), head_dim 8, 64, 128, 256, q written or not
  v_group_kernel                         the same test at 8, 9 and 70 tokens with v_group_append on (7 and
                                         below, and the knob off, take the per-token V append)
  attn_decode_kernel<FUSED>              test_decode_rope_appends_exact_k_and_v
  silu_mul_kernel                        test_silu_mul_exhaustive, (2049, 2048) past the grid cap
  embedding_kernel                       test_embedding: hidden 2056 / 8192 (second loop trip), the clamp
  add_inplace_kernel                     test_add_inplace: 8 (2048 * 256 + 1) elements past the grid cap
  argmax_kernel                          test_argmax_ignores_the_row_padding: row_stride > vocab"""
import math

import pytest
import torch

import gemm_exact_cases as gx
import pertoken_cases as pc
from distributed_llms_amd import _ext, knobs, ops
from distributed_llms_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16, I16 = torch.bfloat16, torch.int16
G = gx.GUARD_ROWS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _unchanged(dev, host, what):
    assert torch.equal(dev.cpu().contiguous().view(I16), host.contiguous().view(I16)), f"{what} was written"


def _guards(buf, rows, what):
    gx.assert_untouched(buf[:G], what + ": rows before the output")
    gx.assert_untouched(buf[G + rows:], what + ": rows after the output")


# ---------------------------------------------------------------- 1. RMSNorm
def _norm_ok(y, ref64, kinds, zero_row):
    msg = pc.rel_mismatch(y, ref64, kinds=kinds)
    assert msg is None, msg
    assert bool((y[zero_row] == 0).all()), "the all-zero row must come out as zeros"


@pytest.mark.parametrize("hidden", pc.NORM_HIDDEN)
def test_rms_norm(cuda, hidden):
    """Random, needle, all-zero and tiny rows within (2^-8 + 2^-12) |ref| of fp64; y between guard rows;
    x and w unchanged; ops.rms_norm gives the same bits."""
    c = pc.norm_case(hidden)
    rows = c.x.shape[0]
    x, w = c.x.cuda(), c.w.cuda()
    buf, y = gx.sentinel_out(rows, hidden)
    _ext.kernels().rms_norm(y.data_ptr(), x.data_ptr(), 0, w.data_ptr(), rows, hidden, pc.EPS, _stream())
    _norm_ok(y, c.ref, c.kinds, c.kinds.index("zero"))
    _guards(buf, rows, "y")
    _unchanged(x, c.x, "x")
    _unchanged(w, c.w, "w")
    pc.assert_same_bits(ops.rms_norm(x, w, pc.EPS), y)


@pytest.mark.parametrize("hidden", pc.NORM_HIDDEN)
def test_fused_add_rms_norm(cuda, hidden):
    """The new residual is bf16(x + res) bit for bit (the sum is exact in f32: cancellations to +0, ties to
    even), the normed output within the rule of the fp64 norm of that residual; y and the residual
    between guard rows; x and w unchanged; ops.fused_add_rms_norm gives the same bits."""
    c = pc.norm_case(hidden)
    rows = c.fx.shape[0]
    x, w = c.fx.cuda(), c.w.cuda()
    ybuf, y = gx.sentinel_out(rows, hidden)
    rbuf, res = gx.sentinel_out(rows, hidden)
    res.copy_(c.fres)
    _ext.kernels().rms_norm(y.data_ptr(), x.data_ptr(), res.data_ptr(), w.data_ptr(), rows, hidden, pc.EPS, _stream())
    pc.assert_same_bits(res, c.new_res)
    _norm_ok(y, c.fref, c.fkinds, c.fkinds.index("zero"))
    _guards(ybuf, rows, "y")
    _guards(rbuf, rows, "residual")
    _unchanged(x, c.fx, "x")
    _unchanged(w, c.w, "w")
    rbuf2, res2 = gx.sentinel_out(rows, hidden)
    res2.copy_(c.fres)
    y2, r2 = ops.fused_add_rms_norm(x, res2, w, pc.EPS)
    assert r2.data_ptr() == res2.data_ptr()
    pc.assert_same_bits(y2, y)
    pc.assert_same_bits(res2, c.new_res)
    _guards(rbuf2, rows, "residual (ops)")


# ---------------------------------------------------------------- 2. rope_cache_append
def _sent_cache(shape):
    return torch.full(shape, pc.SENT16, dtype=I16, device="cuda")


def _gather(cache, idx, shape):
    return cache.view(-1)[idx.reshape(-1).cuda()].view(shape)


def _only_addressed_written(cache, idx, what):
    rest = cache.clone().view(-1)
    rest[idx.reshape(-1).cuda()] = pc.SENT16
    bad = (rest != pc.SENT16).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements outside the tokens' slots written, first {bad[0].item()}"


@pytest.mark.parametrize("kind", pc.ROPE_TABLES)
@pytest.mark.parametrize("tokens", pc.ROPE_TOKENS)
@pytest.mark.parametrize("hq,hkv,d,bs", pc.ROPE_SHAPES)
def test_rope_cache_append(cuda, hq, hkv, d, bs, tokens, kind):
    """Grouped V append on and off, q written or not.  Dyadic table and no table: q, k and v bit for bit,
    the whole caches equal to the expected ones (sentinels wherever no token writes).  Real tables (plain
    and llama3-scaled): q and k within 2^-8 |ref| + 2^-22 (|a c| + |b s|) of fp64, v bit for bit, every
    element no token addresses still the sentinel.  qkv, positions, slots and the table unchanged."""
    c = pc.rope_case(hq, hkv, d, bs, tokens, kind)
    qkv, pos, slots = c.qkv.cuda(), c.pos.cuda(), c.slots.cuda()
    table = None if c.table is None else c.table.cuda()
    exact = kind in ("dyadic", "none")
    for grouped in (True, False):
        for write_q in (True, False):
            kc, vc = _sent_cache(c.k_cache.shape), _sent_cache(c.v_cache.shape)
            with knobs.override(v_group_append=grouped):
                q = ops.rope_cache_append(qkv, pos, table, kc.view(BF16), vc.view(BF16), slots, hq, hkv, d,
                                          write_q=write_q)
            what = f"grouped={grouped} write_q={write_q}"
            assert torch.equal(vc, c.v_cache.cuda()), what + ": v_cache"
            if write_q:
                assert q.shape == (tokens, hq, d)
            else:
                assert q is None
            if exact:
                assert torch.equal(kc, c.k_cache.cuda()), what + ": k_cache: " + str(
                    pc.same_bits(_gather(kc, c.kidx, c.k.shape).view(BF16), c.k))
                if write_q:
                    pc.assert_same_bits(q, c.q)
            else:
                _only_addressed_written(kc, c.kidx, what + ": k_cache")
                msg = pc.rope_real_mismatch(_gather(kc, c.kidx, c.k.shape).view(BF16), c.k64, c.k_slack)
                assert msg is None, what + ": k: " + msg
                if write_q:
                    msg = pc.rope_real_mismatch(q, c.q64, c.q_slack)
                    assert msg is None, what + ": q: " + msg
    _unchanged(qkv, c.qkv, "qkv")
    assert torch.equal(pos.cpu(), c.pos) and torch.equal(slots.cpu(), c.slots)
    if table is not None:
        assert torch.equal(table.cpu(), c.table)


@pytest.mark.parametrize("lens", pc.DECODE_LENS)
@pytest.mark.parametrize("hq,hkv,d", pc.DECODE_SHAPES)
def test_decode_rope_appends_exact_k_and_v(cuda, hq, hkv, d, lens):
    """paged_attention_decode_rope with the dyadic table: the k it appends -- rotated as
    fmaf(a, c, -(b s)), exact here too -- and the v equal the expectation bit for bit, every other cache
    element keeps its bits, and the attention output stays within the bound of
    test_kernels_gpu.test_paged_attention_decode_fused_rope."""
    c = pc.decode_rope_case(hq, hkv, d, tuple(lens))
    k1, v1, bt, sl = c.k0.cuda(), c.v0.cuda(), c.block_tables.cuda(), c.seq_lens.cuda()
    scale = 1 / math.sqrt(d)
    out = ops.paged_attention_decode_rope(c.qkv.cuda(), c.pos.cuda(), c.table.cuda(), k1, v1, c.slots.cuda(), bt, sl,
                                          hq, hkv, d, scale)
    pc.assert_same_bits(k1, c.k_cache)
    pc.assert_same_bits(v1, c.v_cache)
    expect = ref.paged_attention_decode(c.q.float(), c.k_cache.float(), c.v_cache.float(), c.block_tables, c.seq_lens,
                                        scale)
    torch.testing.assert_close(out.float().cpu(), expect, atol=2e-2, rtol=2e-2)


# ---------------------------------------------------------------- 3. silu_mul
@pytest.mark.parametrize("t,inter", pc.SILU_SHAPES)
def test_silu_mul_exhaustive(cuda, t, inter):
    """Every bf16 gate bit pattern times 8 up values: within rtol 2^-8 + 2^-12, atol 1e-30 of fp64
    g sigmoid(g) u where that is finite, the bits of its bf16 (NaN matching NaN) at NaN and infinite gates
    and overflows.  The output between guard rows, the input unchanged.  The share of outputs equal to the
    correctly rounded reference is printed, not asserted (99.96 % for an f32 evaluation with exp and a
    true division; the kernel has __expf and the hardware reciprocal)."""
    c = pc.silu_case(t, inter)
    gu = c.gu.cuda()
    buf, y = gx.sentinel_out(t, inter)
    _ext.kernels().silu_mul(y.data_ptr(), gu.data_ptr(), t, inter, _stream())
    print(f"silu_mul ({t}, {inter}): {100 * pc.rn_share(y, c):.4f} % of the finite outputs equal RN(ref)")
    msg = pc.silu_mismatch(y, c)
    assert msg is None, msg
    _guards(buf, t, "out")
    _unchanged(gu, c.gu, "gu")
    pc.assert_same_bits(ops.silu_mul(gu), y)


# ---------------------------------------------------------------- 4. embedding, add_, argmax
@pytest.mark.parametrize("hidden", pc.EMB_HIDDEN)
def test_embedding(cuda, hidden):
    """Rows gathered bit for bit (compared as int16), ids below 0 and beyond the table clamped to rows 0 and
    vocab - 1, the output between guard rows, ids and the table unchanged."""
    c = pc.embedding_case(hidden)
    table, ids = c.table.cuda(), c.ids.cuda()
    n = ids.numel()
    buf, out = gx.sentinel_out(n, hidden)
    _ext.kernels().embedding(out.data_ptr(), ids.data_ptr(), table.data_ptr(), n, hidden, pc.EMB_VOCAB, _stream())
    pc.assert_same_bits(out, c.expected)
    _guards(buf, n, "out")
    _unchanged(table, c.table, "table")
    assert torch.equal(ids.cpu(), c.ids)
    pc.assert_same_bits(ops.embedding(ids, table), c.expected)


@pytest.mark.parametrize("n", pc.ADD_N)
def test_add_inplace(cuda, n):
    """ops.add_: a <- bf16(a + b) bit for bit (the f32 sum is exact; b = -a gives +0, ties go to even), b
    unchanged, guard rows around a."""
    c = pc.add_case(n)
    buf, a = gx.sentinel_out(n // 8, 8)
    a.copy_(c.a)
    b = c.b.cuda()
    assert ops.add_(a, b).data_ptr() == a.data_ptr()
    pc.assert_same_bits(a, c.expected)
    _guards(buf, n // 8, "a")
    _unchanged(b, c.b, "b")


@pytest.mark.parametrize("pad", pc.ARGMAX_PAD)
@pytest.mark.parametrize("vocab", pc.ARGMAX_VOCAB)
def test_argmax_ignores_the_row_padding(cuda, vocab, pad):
    """Logits are the [:, :vocab] view of rows of pitch vocab + 24 / vocab + 3 (rows that are not 16-byte
    aligned take the scalar scan) whose padding is above every in-vocabulary value."""
    buf, expected = pc.argmax_case(vocab, pad)
    dev = buf.cuda()
    logits = dev[:, :vocab]
    assert logits.stride(0) == vocab + pad
    assert torch.equal(ops.argmax(logits).cpu(), expected)
    _unchanged(dev, buf, "logits")
