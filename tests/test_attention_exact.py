"""Position-exact paged attention: inputs whose expected output changes when ONE key is lost, doubled
or leaks in, so an off-by-one mask, a dropped new key or a stale slot is seen at any context length.

Two input forms, every value exact in bf16 (H: the Sylvester Hadamard matrix of order head_dim):

  needle  q of head g of a GQA group is H[1 + g]; a needle for head g at key p is K[p] += 4 H[1 + g];
          every other K is 0 and V is random.  With the scale 1 / sqrt(d) a needle scores
          4 sqrt(d) >= 32 against 0, so a head returns the mean of V over the needles it may see
          (the uniform mean of V where it sees none); everything else leaks at most n e^-32.
  census  K = 0, q random, V[j] = e_{j mod d}: every probability is 1 and the output is
          count(j = r mod d) / n -- one key more or less moves an entry by 1 / n.

Poison (finite: a masked probability of 0 times NaN is NaN in the P.V MFMA) fills every slot no
sequence owns, the tail of each last block, the blocks in no table, the dedicated block the table
padding points at and, for the fused decode, the new key's slot before the call.  It scores twice a
needle for every head with V = 1024 (needle) or is K = 0, V = 4096 (census).

Expected values: dense fp64 attention over the logical (unpaged) K / V, so the kernels' block-table
walk is checked independently of ops.reference.paged_*.

Tolerance, derived: probabilities are 0 or 1 in bf16 (or below e^-32) and the accumulation is exact
to f32, so the only rounding is the final f32 normalisation and the bf16 store, at most one bf16 ulp
(2^-7 relative) from the fp64 value; leak and f32 accumulation stay below
4200 e^-32 1024 + 2^-24 5 < 1e-5 absolute.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from distributed_llms_amd import knobs, ops
from distributed_llms_amd.ops import reference as ref

BS = 32
RTOL, ATOL = 2.0 ** -7, 1e-5
SCRATCH_BLOCK, PAD_BLOCK = 0, 1     # slot 0 of padded graph rows; where the table padding points
BF = torch.bfloat16

DECODE_HEADS = [(32, 8, 128), (12, 2, 128), (16, 1, 128), (12, 12, 64)]   # G = 4; 6 (wpb 2); 16 (wpb 1); 1
DECODE_CTX = (1, 31, 32, 33, 64, 65, 2048, 2049, 4200)
PREFILL_HEADS = [(32, 8, 128), (8, 4, 128), (32, 2, 128), (12, 12, 64)]   # G = 4, 2, 16, 1
PREFILL_PAIRS = ((37, 37), (64, 64), (65, 65), (128, 64), (300, 1), (2300, 900))   # (ctx, q_len)
FORMS = ["needle", "census"]


def assert_exact(got, expect):
    """The one assertion of this file: ``got`` against the dense fp64 ``expect``."""
    torch.testing.assert_close(got.double().cpu(), expect.cpu(), rtol=RTOL, atol=ATOL)


def hadamard(d):
    h = torch.ones(1, 1)
    while h.shape[0] < d:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def dense(q, k, v, qpos0=None):
    """fp64 attention of q [ql, hq, d] over the logical k / v [hkv, n, d]; query row t sees the keys
    0 .. qpos0 + t (None: all of them).  A row that sees no key gives zeros."""
    ql, hq, d = q.shape
    hkv, n, _ = k.shape
    qf = q.double().view(ql, hkv, hq // hkv, d)
    dev = q.device
    see = torch.ones(ql, n, dtype=torch.bool, device=dev) if qpos0 is None else \
        torch.arange(n, device=dev)[None, :] <= qpos0 + torch.arange(ql, device=dev)[:, None]
    out = []
    for h in range(hkv):                                   # one kv head at a time: bounds the score matrix
        s = torch.einsum("qgd,nd->gqn", qf[:, h], k[h].double()) / math.sqrt(d)
        p = torch.softmax(s.masked_fill(~see, float("-inf")), -1).nan_to_num(0.0)
        out.append(torch.einsum("gqn,nd->qgd", p, v[h].double()))
    return torch.stack(out, 1).reshape(ql, hq, d)


# ------------------------------------------------------------------ builders (CPU tensors)
def _poison(form, hq, hkv, d):
    if form == "needle":
        return 8 * hadamard(d)[1:1 + hq // hkv].sum(0), 1024.0
    return torch.zeros(d), 4096.0


def _logical(form, n, hq, hkv, d, heads, pos, gen):
    """K / V [hkv, n, d] of one sequence; needle form: head heads[i] gets a needle at key pos[i]."""
    g = hq // hkv
    k = torch.zeros(hkv, n, d)
    if form == "needle":
        k.index_put_((heads // g, pos), 4 * hadamard(d)[1 + heads % g], accumulate=True)
        v = torch.randn(hkv, n, d, generator=gen)
    elif form == "census":
        v = torch.eye(d)[torch.arange(n) % d].expand(hkv, n, d)
    else:                                                   # "random": the usual randn regime
        k = torch.randn(hkv, n, d, generator=gen)
        v = torch.randn(hkv, n, d, generator=gen)
    return k.to(BF), v.to(BF).contiguous()


def _queries(form, rows, hq, hkv, d, gen):
    if form == "needle":
        return hadamard(d)[1 + torch.arange(hq) % (hq // hkv)].expand(rows, hq, d).to(BF).contiguous()
    return torch.randn(rows, hq, d, generator=gen).to(BF)


def _page(c, ks, vs, hkv, d, width, gen, skip_last=False):
    """Scatter the logical K / V into a poisoned paged cache through a shuffled block table
    (``skip_last``: all but each sequence's newest key, whose slot keeps the poison)."""
    lens = torch.tensor([k.shape[1] for k in ks])
    b = len(ks)
    nblk = (lens + BS - 1) // BS
    width = width or int(nblk.max())
    nb_total = 2 + int(nblk.sum()) + 3                     # scratch, padding, owned, three in no table
    c.k = c.pk.to(BF).expand(nb_total, hkv, BS, d).contiguous()
    c.v = torch.full((nb_total, hkv, d, BS), c.pv, dtype=BF)
    owned = 2 + torch.randperm(nb_total - 2, generator=gen)[: int(nblk.sum())]
    seq = torch.repeat_interleave(torch.arange(b), nblk)
    c.bt = torch.full((b, width), PAD_BLOCK, dtype=torch.int32)
    c.bt[seq, torch.arange(len(seq)) - (nblk.cumsum(0) - nblk)[seq]] = owned.to(torch.int32)
    nkeys = lens - 1 if skip_last else lens
    seq = torch.repeat_interleave(torch.arange(b), nkeys)
    p = torch.arange(len(seq)) - (nkeys.cumsum(0) - nkeys)[seq]
    slots = (c.bt[seq, p // BS].long() * BS + p % BS).to(torch.int32)
    rows = torch.cat([torch.cat([k[:, :m].transpose(0, 1).reshape(m, hkv * d),
                                 v[:, :m].transpose(0, 1).reshape(m, hkv * d)], 1)
                      for k, v, m in zip(ks, vs, nkeys.tolist())])
    if len(rows):
        ref.rope_cache_append(rows, p.to(torch.int32), None, c.k, c.v, slots, 0, hkv, d)
    c.lens = lens.tolist()
    c.sl = lens.to(torch.int32)
    last = lens - 1
    c.new_slots = (c.bt[torch.arange(b), last // BS].long() * BS + last % BS).to(torch.int32)
    c.ks, c.vs = ks, vs


def decode_needle_positions(ctx, split_len):
    cand = {0, 31, 32, 63, 64, 2047, 2048, split_len - 1, split_len, ctx - 33, ctx - 32, ctx - 2, ctx - 1}
    return sorted(p for p in cand if 0 <= p < ctx)


@functools.lru_cache(maxsize=None)
def decode_case(form, hq, hkv, d, lens, split_len, width=None, fused=False):
    """One decode batch.  Needles: key j of a sequence's candidate list goes to head (j + i) % hq, so
    every candidate key carries a needle and every head has one; two heads of a group may share a key."""
    gen = torch.Generator().manual_seed(len(lens) * 1000 + hq + d + fused)
    c = SimpleNamespace(form=form, hq=hq, hkv=hkv, d=d, fused=fused, split_len=split_len)
    c.pk, c.pv = _poison(form, hq, hkv, d)
    ks, vs = [], []
    for i, n in enumerate(lens):
        cand = torch.tensor(decode_needle_positions(n, split_len))
        j = torch.arange(max(len(cand), hq))
        k, v = _logical(form, n, hq, hkv, d, (j + i) % hq, cand[j % len(cand)], gen)
        ks.append(k)
        vs.append(v)
    c.q = _queries(form, len(lens), hq, hkv, d, gen)
    _page(c, ks, vs, hkv, d, width, gen, skip_last=fused)
    if fused:       # the raw qkv projection row: q, then the new (last) key's k and v
        c.qkv = torch.cat([c.q.reshape(len(lens), -1), torch.stack([k[:, -1].reshape(-1) for k in ks]),
                           torch.stack([v[:, -1].reshape(-1) for v in vs])], 1).contiguous()
        c.pos = c.sl - 1
    c.expect = torch.cat([dense(c.q[i:i + 1], k, v) for i, (k, v) in enumerate(zip(ks, vs))])
    return c


def prefill_needle_positions(ctx, qlen):
    q0 = ctx - qlen
    cand = {0, q0 - 1, q0, q0 + 1, q0 + 31, q0 + 32, 63, 64, ctx - 1}
    return sorted(p for p in cand if 0 <= p < ctx)


@functools.lru_cache(maxsize=None)
def prefill_case(form, hq, hkv, d, pairs=PREFILL_PAIRS):
    """One packed prefill batch.  Needles: every head gets the whole candidate set, except the heads
    3, 7, 11, ... which get only the keys after the first query row -- their early rows see no needle
    and return the uniform mean of V."""
    gen = torch.Generator().manual_seed(hq * 7 + d)
    c = SimpleNamespace(form=form, hq=hq, hkv=hkv, d=d, pairs=pairs)
    c.pk, c.pv = _poison(form, hq, hkv, d)
    ks, vs = [], []
    for ctx, qlen in pairs:
        cand = torch.tensor(prefill_needle_positions(ctx, qlen))
        late = cand[cand > ctx - qlen]
        sets = [late if h % 4 == 3 else cand for h in range(hq)]
        heads = torch.cat([torch.full((len(s),), h) for h, s in enumerate(sets)])
        k, v = _logical(form, ctx, hq, hkv, d, heads, torch.cat(sets), gen)
        ks.append(k)
        vs.append(v)
    qlens = [q for _, q in pairs]
    c.q = _queries(form, sum(qlens), hq, hkv, d, gen)
    _page(c, ks, vs, hkv, d, None, gen)
    c.cu = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0)), dtype=torch.int32)
    c.max_q = max(qlens)
    c.pos = torch.cat([torch.arange(n - q, n) for n, q in pairs]).to(torch.int32)
    # q as rows of a qkv projection (strided q); the k / v columns are never read by the prefill kernels
    c.qkv = torch.cat([c.q.reshape(sum(qlens), -1),
                       torch.randn(sum(qlens), 2 * hkv * d, generator=gen).to(BF)], 1).contiguous()
    cu = c.cu.tolist()
    c.expect = torch.cat([dense(c.q[cu[i]:cu[i + 1]], ks[i], vs[i], n - q) for i, (n, q) in enumerate(pairs)])
    return c


def _dev(c, *names, dev="cuda"):
    return [getattr(c, n).to(dev) for n in names]


def _default_split_len(b, hkv, width):
    return ops.decode_split_plan(b, hkv, width * BS, BS, width)[1]


def _decode_batch(form, hq, hkv, d, fused=False):
    width = -(-max(DECODE_CTX) // BS)
    return decode_case(form, hq, hkv, d, DECODE_CTX, _default_split_len(len(DECODE_CTX), hkv, width), fused=fused)


# ------------------------------------------------------------------ CPU self-checks
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hq,hkv,d", DECODE_HEADS)
def test_cpu_reference_passes_decode_cases(hq, hkv, d, form):
    """The builders + the fp32 paged reference pass the helper: the construction is what it claims."""
    c = _decode_batch(form, hq, hkv, d)
    scale = 1 / math.sqrt(d)
    assert_exact(ref.paged_attention_decode(c.q.float(), c.k.float(), c.v.float(), c.bt, c.sl, scale), c.expect)
    f = _decode_batch(form, hq, hkv, d, fused=True)
    k2, v2 = f.k.float(), f.v.float()
    q = ref.rope_cache_append(f.qkv.float(), f.pos, None, k2, v2, f.new_slots, hq, hkv, d)
    assert_exact(ref.paged_attention_decode(q, k2, v2, f.bt, f.sl, scale), f.expect)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hq,hkv,d", PREFILL_HEADS)
def test_cpu_reference_passes_prefill_cases(hq, hkv, d, form):
    c = prefill_case(form, hq, hkv, d)
    got = ref.paged_attention_prefill(c.q.float(), c.k.float(), c.v.float(), c.bt, c.cu, c.sl, 1 / math.sqrt(d))
    assert_exact(got, c.expect)


def _with_poison(c, k, v, extra):
    """The logical keys followed by ``extra`` poison keys: what the cache holds past the context."""
    hkv, _, d = k.shape
    return (torch.cat([k, c.pk.to(BF).expand(hkv, extra, d)], 1),
            torch.cat([v, torch.full((hkv, extra, d), c.pv, dtype=BF)], 1))


def _swap_last_block(c, k, v):
    """Swap the last block's id with the next table entry (padding: the poison block)."""
    n = k.shape[1]
    nb = -(-n // BS)
    kp, vp = _with_poison(c, k, v, (nb + 1) * BS - n)
    order = torch.arange((nb + 1) * BS).view(nb + 1, BS)
    order[[nb - 1, nb]] = order[[nb, nb - 1]]
    return kp[:, order.reshape(-1)[:n]], vp[:, order.reshape(-1)[:n]]


def _stale_new_key(c, k, v):
    k, v = k.clone(), v.clone()
    k[:, -1], v[:, -1] = c.pk.to(BF), c.pv
    return k, v


def _drop(k, v, lo, hi):
    keep = torch.ones(k.shape[1], dtype=torch.bool)
    keep[lo:hi] = False
    return k[:, keep], v[:, keep]


DECODE_MUTANTS = {
    "drop key ctx-1": lambda c, k, v: _drop(k, v, k.shape[1] - 1, k.shape[1]),
    "admit key ctx (poison)": lambda c, k, v: _with_poison(c, k, v, 1),
    "drop a 32-key chunk": lambda c, k, v: _drop(k, v, 0, BS),
    "swap two block ids": _swap_last_block,
    "fused: stale slot for the new key": _stale_new_key,
}


@pytest.mark.parametrize("mutant", list(DECODE_MUTANTS))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hq,hkv,d", [(12, 2, 128), (12, 12, 64)])
def test_decode_mutants_are_rejected_at_every_context(hq, hkv, d, form, mutant):
    """A wrong dense attention fails the helper for every sequence of the decode batch, in both forms:
    the tests in this file can fail.

    One documented blind spot: a whole lost chunk moves a census entry by (32 - d) / n or 32 / n
    relative, which is below one ulp from n = 128 max(32, d - 32) keys (4096 at d = 64), so there
    only the needle form (the chunk carries one) has to reject it."""
    c = _decode_batch(form, hq, hkv, d, fused=mutant.startswith("fused"))
    for i, n in enumerate(c.lens):
        if form == "census" and mutant == "drop a 32-key chunk" and n >= 128 * max(32, d - 32):
            continue
        k, v = DECODE_MUTANTS[mutant](c, c.ks[i], c.vs[i])
        with pytest.raises(AssertionError):
            assert_exact(dense(c.q[i:i + 1], k, v), c.expect[i:i + 1])
        assert_exact(dense(c.q[i:i + 1], c.ks[i], c.vs[i]), c.expect[i:i + 1])     # and the unmutated passes


def _admit_poison_prefill(c, q, k, v, q0):
    """Correct diagonal, but the last row's key limit is ctx instead of ctx - 1."""
    return torch.cat([dense(q[:-1], k, v, q0), dense(q[-1:], *_with_poison(c, k, v, 1))])


PREFILL_MUTANTS = {
    "drop key ctx-1": lambda c, q, k, v, q0: dense(q, *_drop(k, v, k.shape[1] - 1, k.shape[1]), q0),
    "admit key ctx (poison)": _admit_poison_prefill,
    "drop a 32-key chunk": lambda c, q, k, v, q0: dense(q, *_drop(k, v, 0, BS), q0 - min(BS, k.shape[1])),
    "swap two block ids": lambda c, q, k, v, q0: dense(q, *_swap_last_block(c, k, v), q0),
    "diagonal one late (row t sees key t+1)": lambda c, q, k, v, q0: dense(q, *_with_poison(c, k, v, 1), q0 + 1),
    "diagonal one early (row t misses key t)": lambda c, q, k, v, q0: dense(q, k, v, q0 - 1),
}


@pytest.mark.parametrize("mutant", list(PREFILL_MUTANTS))
@pytest.mark.parametrize("form", FORMS)
def test_prefill_mutants_are_rejected_at_every_pair(form, mutant):
    c = prefill_case(form, 8, 4, 128)
    cu = c.cu.tolist()
    for i, (n, ql) in enumerate(c.pairs):
        q, want = c.q[cu[i]:cu[i + 1]], c.expect[cu[i]:cu[i + 1]]
        with pytest.raises(AssertionError):
            assert_exact(PREFILL_MUTANTS[mutant](c, q, c.ks[i], c.vs[i], n - ql), want)


# ------------------------------------------------------------------ decode on the GPU
def _run_decode(c, **kw):
    q, k, v, bt, sl = _dev(c, "q", "k", "v", "bt", "sl")
    return ops.paged_attention_decode(q, k, v, bt, sl, 1 / math.sqrt(c.d), **kw)


def _run_fused(c, cos_sin=None, qkv=None, **kw):
    """The fused op on fresh copies of the case's cache -> (out, k, v, expected k, expected v)."""
    qkv0, pos, k, v, slots, bt, sl = _dev(c, "qkv", "pos", "k", "v", "new_slots", "bt", "sl")
    k2, v2 = k.clone(), v.clone()
    ref.rope_cache_append(qkv0, pos, cos_sin, k2, v2, slots, c.hq, c.hkv, c.d)
    out = ops.paged_attention_decode_rope(qkv0 if qkv is None else qkv, pos, cos_sin, k, v, slots, bt, sl, c.hq,
                                          c.hkv, c.d, 1 / math.sqrt(c.d), **kw)
    return out, k, v, k2, v2


def _assert_fused(c, **kw):
    out, k, v, k2, v2 = _run_fused(c, **kw)
    assert_exact(out, c.expect)
    # every slot but the new one as before the call, poison included; the new one as the reference append
    assert torch.equal(k, k2) and torch.equal(v, v2)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hq,hkv,d", DECODE_HEADS)
def test_decode_exact(cuda, hq, hkv, d, form):
    assert_exact(_run_decode(_decode_batch(form, hq, hkv, d)), _decode_batch(form, hq, hkv, d).expect)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hq,hkv,d", DECODE_HEADS)
def test_decode_fused_exact(cuda, hq, hkv, d, form):
    """The new key comes from qkv (its slot holds poison before the call): needles on it for some heads,
    on cached keys for others."""
    _assert_fused(_decode_batch(form, hq, hkv, d, fused=True))


@pytest.mark.gpu
def test_decode_fused_rope_needle_on_new_key(cuda):
    """RoPE given: needles only on the new key -- q and k rotate by the same position, so the margin
    (a needle's score against the unrotated zeros of the cache) survives the rotation's rounding."""
    hq, hkv, d = 32, 8, 128
    lens = DECODE_CTX
    gen = torch.Generator().manual_seed(11)
    c = SimpleNamespace(form="needle", hq=hq, hkv=hkv, d=d)
    c.pk, c.pv = _poison("needle", hq, hkv, d)
    ks, vs = [], []
    for n in lens:
        k, v = _logical("needle", n, hq, hkv, d, torch.arange(hq), torch.full((hq,), n - 1), gen)
        ks.append(k)
        vs.append(v)
    c.q = _queries("needle", len(lens), hq, hkv, d, gen)
    _page(c, ks, vs, hkv, d, None, gen, skip_last=True)
    c.qkv = torch.cat([c.q.reshape(len(lens), -1), torch.stack([k[:, -1].reshape(-1) for k in ks]),
                       torch.stack([v[:, -1].reshape(-1) for v in vs])], 1).contiguous()
    c.pos = c.sl - 1
    c.expect = torch.stack([v[:, -1].double().repeat_interleave(hq // hkv, 0) for v in vs])   # the new v itself
    k0 = c.k.cuda()
    cs = ref.rope_cos_sin(d, 8192, 500000.0, device="cuda")
    out, k, v, k2, v2 = _run_fused(c, cos_sin=cs)
    assert_exact(out, c.expect)
    assert torch.equal(v, v2)
    # the rotated new k: one bf16 ulp (fma or not) and the f32 rounding of products of magnitude <= 64
    torch.testing.assert_close(k.float(), k2.float(), rtol=RTOL, atol=1e-4)
    zero = torch.zeros_like(c.qkv).cuda()
    for t in (k, k0):                                      # every other slot: as before the call
        ref.rope_cache_append(zero, c.pos.cuda(), None, t, v.clone(), c.new_slots.cuda(), hq, hkv, d)
    assert torch.equal(k, k0)


@pytest.mark.gpu
@pytest.mark.parametrize("b,waves,plan", [(1, 1, (1, 4224)), (2, 1, (1, 4224)), (3, 1, (1, 4224)),
                                          (1, 2, (2, 2112)), (3, 8, (2, 2112))])
def test_decode_second_block_id_pass(cuda, b, waves, plan):
    """A split longer than 64 chunks: the kernel reloads its block ids (one split of 132 chunks), also
    from a split that does not start at chunk 0 (two splits of 66)."""
    hq, hkv, d, width = 4, 1, 128, 132
    lens = (4200, 2049, 2112)[:b]
    with knobs.override(attn_target_waves=waves):
        assert ops.decode_split_plan(b, hkv, width * BS, BS, width) == plan     # else the path is not covered
        for form in FORMS:
            c = decode_case(form, hq, hkv, d, lens, plan[1], width)
            assert_exact(_run_decode(c), c.expect)
            _assert_fused(decode_case(form, hq, hkv, d, lens, plan[1], width, fused=True))


ENGINE_LENS = (1, 33, 640, 2049, 300)


def _engine_case(form, fused=False):
    hq, hkv, d, width = 32, 8, 128, 132                    # a table sized for the model's context, mostly padding
    return decode_case(form, hq, hkv, d, ENGINE_LENS, _default_split_len(len(ENGINE_LENS), hkv, width), width, fused)


def _nan_workspace(c, splits):
    n = len(c.lens) * c.hq * splits
    return (torch.full((3 * n * c.d + 7,), float("nan"), device="cuda"),
            torch.full((3 * n * 2 + 7,), float("nan"), device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_decode_max_ctx_and_workspace(cuda, form):
    """max_ctx = the batch's longest context against None (the table's capacity) with an oversized,
    NaN-filled workspace: every partial the reduce reads was written, empty splits included, and the
    two split counts give the same bits."""
    c = _engine_case(form)
    splits = ops.decode_split_plan(len(c.lens), c.hkv, c.bt.shape[1] * BS, BS, c.bt.shape[1])[0]
    assert splits > ops.decode_split_plan(len(c.lens), c.hkv, max(c.lens), BS, c.bt.shape[1])[0] > 1
    a = _run_decode(c, max_ctx=max(c.lens), workspace=_nan_workspace(c, splits))
    b = _run_decode(c, max_ctx=None, workspace=_nan_workspace(c, splits))
    assert_exact(a, c.expect)
    assert_exact(b, c.expect)
    assert torch.equal(a, b)
    f = _engine_case(form, fused=True)
    fa = _assert_fused(f, max_ctx=max(f.lens), workspace=_nan_workspace(f, splits))
    fb = _assert_fused(f, max_ctx=None, workspace=_nan_workspace(f, splits))
    assert torch.equal(fa, fb)


@pytest.mark.gpu
def test_decode_out_slice(cuda):
    """out= a [B, hq, d] slice of a larger buffer: written in place, the rows around it untouched."""
    c = _engine_case("needle")
    b = len(c.lens)
    big = torch.full((b + 5, c.hq, c.d), float("nan"), dtype=BF, device="cuda")
    got = _run_decode(c, out=big[2:2 + b])
    assert got.data_ptr() == big[2].data_ptr()
    assert_exact(big[2:2 + b], c.expect)
    assert big[:2].isnan().all() and big[2 + b:].isnan().all()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_decode_padded_bucket_bit_identical(cuda, form):
    """Batch 5 against the same rows padded to 8 as engine.graphs pads them (one token, position, slot
    and table 0) with max_ctx at the next power of two: the same bits, plain and fused."""
    pad = 3
    pow2 = 1 << (max(ENGINE_LENS) - 1).bit_length()
    scale = 1 / math.sqrt(128)

    def padded(t, fill=0):
        return torch.cat([t, torch.full((pad, *t.shape[1:]), fill, dtype=t.dtype, device=t.device)])

    c = _engine_case(form)
    b = len(c.lens)
    assert pow2 <= c.bt.shape[1] * BS
    q, k, v, bt, sl = _dev(c, "q", "k", "v", "bt", "sl")
    eager = ops.paged_attention_decode(q, k, v, bt, sl, scale, max_ctx=max(c.lens))
    graph = ops.paged_attention_decode(padded(q), k, v, padded(bt), padded(sl, 1), scale, max_ctx=pow2)
    assert_exact(eager, c.expect)
    assert torch.equal(graph[:b], eager)

    f = _engine_case(form, fused=True)
    eager = _assert_fused(f, max_ctx=max(f.lens))
    qkv, pos, k, v, slots, bt, sl = _dev(f, "qkv", "pos", "k", "v", "new_slots", "bt", "sl")
    graph = ops.paged_attention_decode_rope(padded(qkv), padded(pos), None, k, v, padded(slots), padded(bt),
                                            padded(sl, 1), f.hq, f.hkv, f.d, scale, max_ctx=pow2)
    assert torch.equal(graph[:b], eager)


# ------------------------------------------------------------------ prefill on the GPU
_PREFILL_GPU = [(v, h) for h in PREFILL_HEADS for v in (3, 4, 7, 9) if h[2] == 128 or v in (3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("version,heads", _PREFILL_GPU, ids=lambda x: str(x).replace(", ", "-"))
def test_prefill_exact(cuda, version, heads, form):
    """Row t sees a needle at t and not one at t + 1, at every tile edge; the chunked prefill (2300, 900)
    starts mid-block with more than 64 chunks."""
    c = prefill_case(form, *heads)
    q, k, v, bt, cu, sl = _dev(c, "q", "k", "v", "bt", "cu", "sl")
    out = ops.paged_attention_prefill(q, k, v, bt, cu, sl, 1 / math.sqrt(c.d), version=version)
    assert_exact(out, c.expect)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("version", [4, 7, 9])
def test_prefill_strided_q_exact(cuda, version, form):
    """cos_sin=None: q is read in place from the rows of the qkv projection."""
    c = prefill_case(form, 32, 8, 128)
    qkv, pos, k, v, bt, cu, sl = _dev(c, "qkv", "pos", "k", "v", "bt", "cu", "sl")
    with knobs.override(prefill_attn=version, prefill_fused_rope=True):
        out = ops.paged_attention_prefill_rope(qkv, pos, None, k, v, bt, cu, sl, c.hq, c.d, 1 / math.sqrt(c.d),
                                               max_q_len=c.max_q)
    assert_exact(out, c.expect)


@pytest.mark.gpu
def test_prefill_strided_q_with_rope_runs(cuda):
    """cos_sin given (q rotates, the cached K of this construction does not): random K / V at the
    suite's usual 2e-2, only to keep the in-kernel rotation of a strided q running on this batch."""
    c = prefill_case("random", 32, 8, 128)
    qkv, pos, k, v, bt, cu, sl = _dev(c, "qkv", "pos", "k", "v", "bt", "cu", "sl")
    cs = ref.rope_cos_sin(c.d, 4096, 500000.0, device="cuda")
    with knobs.override(prefill_attn=0, prefill_fused_rope=True):
        out = ops.paged_attention_prefill_rope(qkv, pos, cs, k, v, bt, cu, sl, c.hq, c.d, 1 / math.sqrt(c.d),
                                               max_q_len=c.max_q)
    q = ref.rope_q(qkv.float(), pos, cs, c.hq, c.d)
    cl = c.cu.tolist()
    expect = torch.cat([dense(q[cl[i]:cl[i + 1]], c.ks[i].cuda(), c.vs[i].cuda(), n - ql)
                        for i, (n, ql) in enumerate(c.pairs)])
    torch.testing.assert_close(out.double(), expect, atol=2e-2, rtol=2e-2)
