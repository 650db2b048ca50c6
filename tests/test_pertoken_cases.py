"""CPU checks of tests/pertoken_cases.py: every builder precondition the GPU tests of
test_pertoken_exact.py rest on, and the proof that the acceptance rules bite -- each wrong kernel below
is emulated in torch on a case's own inputs and must be rejected, while the correct f32 emulation passes.

Why this file exists: test_kernels_gpu.py holds these kernels to randn inputs with atol = rtol = 2e-2,
and test_old_tolerance_passes_the_first_two_mutants shows that an RMSNorm that leaves the row's last
16-byte vector out of the sum of squares, and one without eps, both pass that check."""
import pytest
import torch

import pertoken_cases as pc
from distributed_llms_amd.ops import reference as ref

BF16 = torch.bfloat16


# ---------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("hidden", pc.NORM_HIDDEN)
def test_norm_case_preconditions(hidden):
    """fx + fres exact in f32, the cancellation and the ties (asserted by the builder); every needle row
    moves by more than 10x when the needle leaves the sum of squares; eps dominates the tiny row; the
    correct f32 evaluation passes the rule with no violation, on both forms."""
    c = pc.norm_case(hidden)
    assert c.x.shape[0] == len(c.kinds) and c.fx.shape[0] == len(c.fkinds)
    cols = pc.needle_columns(hidden)
    assert {0, hidden - 1, hidden // 2}.issubset(cols) and all(0 <= v < hidden for v in cols)
    for rows in (c.x, c.new_res):
        r = rows[3:3 + len(cols)].double()
        ss = r.pow(2).sum(-1)
        without = ss - 64.0 ** 2
        ratio = torch.sqrt((ss / hidden + pc.EPS) / (without / hidden + pc.EPS))
        assert ratio.min().item() > 10, ratio.min().item()
        tiny = rows[4 + len(cols)].double()
        assert 0 < tiny.abs().max() < 2.0 ** -18 and tiny.pow(2).mean().item() < pc.EPS * 1e-5
        assert bool((rows[3 + len(cols)] == 0).all())
    assert pc.rel_mismatch(pc.norm_emulate(c.x, c.w), c.ref, kinds=c.kinds) is None
    assert pc.rel_mismatch(pc.norm_emulate(c.new_res, c.w), c.fref, kinds=c.fkinds) is None
    assert bool((pc.norm_emulate(c.x, c.w)[3 + len(cols)] == 0).all())
    torch.testing.assert_close(c.ref.float(), ref.rms_norm(c.x.float(), c.w.float(), pc.EPS), rtol=1e-4, atol=0)


@pytest.mark.parametrize("hidden", pc.NORM_HIDDEN)
@pytest.mark.parametrize("mutant", ["drop_last_vector", "no_eps", "mean_over", "truncate"])
def test_norm_rule_rejects_wrong_kernels(hidden, mutant):
    """A mean over hidden + 8 scales a row by sqrt(hidden / (hidden + 8)), 1 - 4 / hidden: at 16384 that is
    2^-12, the f32 slack of the rule itself, so the rule cannot tell it there; up to 8200 it does."""
    if mutant == "mean_over" and hidden == 16384:
        assert 1 - (hidden / (hidden + 8.0)) ** 0.5 < 2.0 ** -12
        return
    c = pc.norm_case(hidden)
    kw = {mutant: (hidden + 8 if mutant == "mean_over" else True)}
    assert pc.rel_mismatch(pc.norm_emulate(c.x, c.w, **kw), c.ref, kinds=c.kinds) is not None
    assert pc.rel_mismatch(pc.norm_emulate(c.new_res, c.w, **kw), c.fref, kinds=c.fkinds) is not None


def test_old_tolerance_passes_the_first_two_mutants():
    """randn at hidden 4096 under atol = rtol = 2e-2 (test_kernels_gpu.test_rms_norm): dropping the last
    vector from the sum of squares and omitting eps both pass."""
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(7, 4096, generator=g).to(BF16), torch.randn(4096, generator=g).to(BF16)
    yr = ref.rms_norm(x.float(), w.float(), pc.EPS)
    for kw in ({"drop_last_vector": True}, {"no_eps": True}):
        torch.testing.assert_close(pc.norm_emulate(x, w, **kw).float(), yr, atol=2e-2, rtol=2e-2)


# ---------------------------------------------------------------- rope_cache_append
ROPE_ALL = [s + (t, k) for s in pc.ROPE_SHAPES for t in pc.ROPE_TOKENS for k in pc.ROPE_TABLES]


@pytest.mark.parametrize("hq,hkv,d,bs,tokens,kind", ROPE_ALL)
def test_rope_case_preconditions(hq, hkv, d, bs, tokens, kind):
    """Slots and positions in range and slots distinct (asserted by the builder, with the dyadic exactness
    and the rounded share); the expected caches agree with the project's reference scatter; the f32
    evaluation passes the case's rule."""
    c = pc.rope_case(hq, hkv, d, bs, tokens, kind)
    assert int(c.pos.min()) >= 0 and int(c.pos.max()) < pc.MAX_POS
    assert int(c.slots.min()) >= 0 and int(c.slots.max()) < pc.ROPE_BLOCKS * bs
    assert c.slots.unique().numel() == tokens
    k2 = torch.full((pc.ROPE_BLOCKS, hkv, bs, d), pc.SENT16, dtype=torch.int16).view(BF16)
    v2 = torch.full((pc.ROPE_BLOCKS, hkv, d, bs), pc.SENT16, dtype=torch.int16).view(BF16)
    q2 = ref.rope_cache_append(c.qkv, c.pos, c.table, k2, v2, c.slots, hq, hkv, d)
    assert torch.equal(v2.view(torch.int16), c.v_cache)
    x = c.qkv.view(tokens, hq + 2 * hkv, d)
    q32, k32 = pc.rotate32(x[:, :hq], c.pos, c.table), pc.rotate32(x[:, hq:hq + hkv], c.pos, c.table)
    if kind in ("dyadic", "none"):
        assert torch.equal(k2.view(torch.int16), c.k_cache) and pc.same_bits(q2, c.q) is None
        assert pc.same_bits(q32, c.q) is None and pc.same_bits(k32, c.k) is None
    else:
        assert pc.rope_real_mismatch(q32, c.q64, c.q_slack) is None
        assert pc.rope_real_mismatch(k32, c.k64, c.k_slack) is None
        assert pc.rope_real_mismatch(k2.view(-1)[c.kidx.reshape(-1)].view(c.k64.shape), c.k64, c.k_slack) is None


def test_rope_slot_pattern():
    """At 70 tokens every offset of a block occurs, and the groups of 8 tokens are of every kind the
    grouped V append tells apart."""
    for bs in (16, 32):
        sl = pc.rope_slots(70, bs)
        assert {s % bs for s in sl} == set(range(bs))
        groups = [sl[i:i + 8] for i in range(0, 70, 8)]
        consecutive = [len(gr) == 8 and all(gr[j] == gr[0] + j for j in range(8)) for gr in groups]
        assert consecutive[0] and groups[0][0] % 8 == 0                              # aligned whole group
        assert consecutive[5] and groups[5][0] % 8 == 4                              # starts mid-group
        assert not consecutive[6] and sorted(groups[6]) == list(range(5 * bs, 5 * bs + 8))
        assert consecutive[7] and groups[7][0] // bs != groups[7][7] // bs           # across a block boundary
        assert len(groups[8]) == 6
    assert pc.rope_slots(8, 32) == list(range(24, 32)) and pc.rope_slots(9, 32)[-1] == 32
    pos = pc.rope_positions(70)
    assert 0 in pos and pc.MAX_POS - 1 in pos and len(set(pos)) < 70 and pos != sorted(pos)
    assert pc.rope_positions(1) == [pc.MAX_POS - 1]


@pytest.mark.parametrize("d", [8, 64, 128, 256])
def test_dyadic_table_neighbours_differ(d):
    t = pc.rope_table("dyadic", d)
    assert bool((t[1:].abs() != t[:-1].abs()).all())
    assert bool((t[:, 1:d // 2].abs() != t[:, :d // 2 - 1].abs()).all())
    assert bool((t[:, d // 2 + 1:].abs() != t[:, d // 2:-1].abs()).all())
    e = torch.log2(t.abs())
    assert bool((e == e.round()).all()) and e.min() == -3 and e.max() == 3
    assert bool((t < 0).any()) and bool((t > 0).any())


@pytest.mark.parametrize("hq,hkv,d,bs", pc.ROPE_SHAPES)
def test_rope_rules_reject_wrong_kernels(hq, hkv, d, bs):
    """Row pos + 1, pair p + 1 and a truncating store against the exact (dyadic) rule and, for the store,
    the real-table rule; krow32 as the identity and the V^T order of the other block size against the
    expected caches."""
    t = 70
    c = pc.rope_case(hq, hkv, d, bs, t, "dyadic")
    xk = c.qkv.view(t, hq + 2 * hkv, d)[:, hq:hq + hkv]
    for kw in ({"pos_shift": 1}, {"pair_shift": 1}):
        wrong = pc.rotate64(xk, c.pos, c.table, **kw)[0].to(BF16)
        assert (wrong.view(torch.int16) != c.k.view(torch.int16)).double().mean().item() > 0.5
    assert pc.same_bits(pc.rotate32(xk, c.pos, c.table, truncate=True), c.k) is not None
    r = pc.rope_case(hq, hkv, d, bs, t, "real")
    assert pc.rope_real_mismatch(pc.rotate32(xk, r.pos, r.table, truncate=True), r.k64, r.k_slack) is not None
    for kw in ({"pos_shift": 1}, {"pair_shift": 1}):
        if d > 8 or "pos_shift" in kw:
            wrong = pc.rotate64(xk, r.pos, r.table, **kw)[0].to(BF16)
            assert pc.rope_real_mismatch(wrong, r.k64, r.k_slack) is not None
    shape_k, shape_v = (pc.ROPE_BLOCKS, hkv, bs, d), (pc.ROPE_BLOCKS, hkv, d, bs)
    kidx, vidx = pc.cache_indices(c.slots, hkv, d, bs, krow_identity=True, other_vofs=True)
    if bs == 32:
        assert not torch.equal(pc.fill_cache(shape_k, kidx, c.k), c.k_cache)
    else:
        assert torch.equal(kidx, c.kidx)                   # plain rows are the layout of other block sizes
    assert int(vidx.max()) < c.v_cache.numel()
    assert not torch.equal(pc.fill_cache(shape_v, vidx, c.v), c.v_cache)


@pytest.mark.parametrize("hq,hkv,d", pc.DECODE_SHAPES)
@pytest.mark.parametrize("lens", pc.DECODE_LENS)
def test_decode_rope_case_preconditions(hq, hkv, d, lens):
    """The fmaf(a, c, -(b s)) form is exact (asserted by the builder); the expected caches are the
    reference's append into the previous contents; slots are the last position of each sequence."""
    c = pc.decode_rope_case(hq, hkv, d, tuple(lens))
    k2, v2 = c.k0.clone(), c.v0.clone()
    ref.rope_cache_append(c.qkv, c.pos, c.table, k2, v2, c.slots, hq, hkv, d)
    assert torch.equal(k2.view(torch.int16), c.k_cache.view(torch.int16))
    assert torch.equal(v2.view(torch.int16), c.v_cache.view(torch.int16))
    changed = (c.k_cache.view(torch.int16) != c.k0.view(torch.int16)).sum().item()
    assert 0.9 * len(lens) * hkv * d <= changed <= len(lens) * hkv * d
    for i, n in enumerate(lens):
        assert int(c.slots[i]) == int(c.block_tables[i, (n - 1) // 32]) * 32 + (n - 1) % 32


# ---------------------------------------------------------------- silu_mul
def test_silu_pairs_bookkeeping():
    """524 288 pairs, every gate pattern with every up value; the non-finite class is the NaN gates, +-inf
    and the overflows, and nothing else."""
    gate, up, r, finite, expected = pc.silu_pairs()
    assert gate.numel() == pc.SILU_PAIRS and gate.view(torch.int16).unique().numel() == 65536
    assert up.unique().numel() == 8 and bool((up.view(8, 65536) == up.view(8, 65536)[:, :1]).all())
    g = gate.float()
    nan, pinf, ninf = torch.isnan(g), g == float("inf"), g == float("-inf")
    assert nan.sum().item() == 8 * 254 and pinf.sum().item() == 8 and ninf.sum().item() == 8
    assert bool(torch.isnan(r[nan | ninf]).all()) and bool(torch.isinf(r[pinf]).all())
    other = ~finite & ~(nan | pinf | ninf)
    assert bool((r[other].abs() >= pc.BF16_MAX).all()) and bool((g[other] > 2.0 ** 126).all())
    assert finite.sum().item() + (~finite).sum().item() == pc.SILU_PAIRS
    assert (~finite).sum().item() == 8 * 256 + other.sum().item() and 0 < other.sum().item() < 200
    assert finite.sum().item() == 522100 and (~finite).sum().item() == 2188
    at_max = r[other].abs() == pc.BF16_MAX                        # the maximum itself: 4 pairs, stored as it is
    assert at_max.sum().item() == 4 and bool((torch.isinf(expected[other].float()) | at_max).all())


@pytest.mark.parametrize("t,inter", pc.SILU_SHAPES)
def test_silu_case_and_rule(t, inter):
    """Each tiling holds every pair -- (255, 2056) all but the last 8, NaN gates that the others hold -- and
    the last needs more than the 2048 x 256 grid's vectors; the f32 emulation of the kernel's formula
    passes; truncation and a clamped exp fail."""
    c = pc.silu_case(t, inter)
    assert c.gu.shape == (t, 2 * inter) and t * inter >= pc.SILU_PAIRS - 8 and inter % 8 == 0
    if (t, inter) == pc.SILU_SHAPES[-1]:
        assert t * inter // 8 > 2048 * 256
    y = pc.silu_emulate(c.gu)
    assert pc.silu_mismatch(y, c) is None
    assert pc.rn_share(y, c) > 0.99
    assert pc.silu_mismatch(pc.silu_emulate(c.gu, truncate=True), c) is not None
    assert pc.silu_mismatch(pc.silu_emulate(c.gu, clamp=20.0), c) is not None


# ---------------------------------------------------------------- embedding, add_, argmax
@pytest.mark.parametrize("hidden", pc.EMB_HIDDEN)
def test_embedding_case(hidden):
    c = pc.embedding_case(hidden)
    t = c.table.view(torch.int16)
    assert all(t[r].unique().numel() == hidden for r in (0, 1, pc.EMB_VOCAB - 1))
    assert all(t[:, col].unique().numel() == pc.EMB_VOCAB for col in (0, hidden - 1))
    ids = c.ids.tolist()
    assert {0, pc.EMB_VOCAB - 1, -1, -2 ** 31, pc.EMB_VOCAB, 2 ** 31 - 1}.issubset(ids) and len(set(ids)) < len(ids)
    e = c.expected.view(torch.int16)
    assert torch.equal(e[-4], t[0]) and torch.equal(e[-3], t[0])
    assert torch.equal(e[-2], t[-1]) and torch.equal(e[-1], t[-1])
    assert torch.equal(e[:-4], ref.embedding(c.ids[:-4], c.table).view(torch.int16))


@pytest.mark.parametrize("n", pc.ADD_N)
def test_add_case(n):
    """The f32 sum is exact (asserted by the builder); cancellations and ties are there; a truncating
    store is rejected."""
    c = pc.add_case(n)
    assert c.a.numel() == n and c.ties >= 0.1
    q = max(1, n // 4)
    assert bool((c.expected.view(-1)[:q] == 0).all())
    s = c.a.float() + c.b.float()
    assert pc.same_bits(s.to(BF16), c.expected) is None
    assert pc.same_bits(pc.trunc_bf16(s), c.expected) is not None
    if n == pc.ADD_N[-1]:
        assert n // 8 > 2048 * 256


@pytest.mark.parametrize("vocab", pc.ARGMAX_VOCAB)
@pytest.mark.parametrize("pad", pc.ARGMAX_PAD)
def test_argmax_case(vocab, pad):
    buf, expected = pc.argmax_case(vocab, pad)
    assert bool((buf.float().argmax(-1) >= vocab).all())          # a kernel that scans the pitch picks padding
    assert bool((expected < vocab).all()) and buf.stride(0) == vocab + pad
    assert torch.equal(expected, ref.argmax(buf[:, :vocab]))
