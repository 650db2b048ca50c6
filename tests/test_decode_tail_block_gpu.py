"""Decode attention loads only the context's keys from the last KV block (attention.hip load_chunk_rows).

The last 32-key block of a (sequence, split) holds ``nadm`` admissible cache keys: keys <= kmax, and in
the fused kernel keys < ctx - 1 (the new key comes from registers).  The kernel ends its buffer
descriptors behind them, so the stale K rows and V^T groups of that block are never requested and their
registers hold zeros.  Checked here, at Hq 8 / Hkv 2 (G = 4) / D 128 / B 3 and contexts 1, 2, 8, 9, 31,
32, 33, 40, 63, 64, 65, 97 (new-key offsets 0, 7, 8, 30, 31; a tail of one key and a full tail; the tail
in the first and in a later block), fused with bf16 qkv and with 3 and 5 split-K slabs and unfused, with
one split, with the tail chunk alone in its split (split length 32) and with the planner's split length:

* every cache slot at or beyond the admissible keys, and every block no sequence owns (block 0, which
  the padded block-table entries name, included), holds a large finite poison: the output matches the
  fp32 reference over the admissible keys at the tolerance of test_kernels_gpu's decode tests;
* the same call with that tail zeroed gives the same output bits;
* fused: afterwards the cache equals, bit for bit, the cache ``rope_cache_append`` leaves -- the new
  key's K row and V^T values, every earlier key, and the stale slots as well (the whole-line V^T
  write-back rewrites the new key's 8-key group, which is therefore loaded even when none of its
  keys is admissible yet: test_pertoken_exact.test_decode_rope_appends_exact_k_and_v and
  test_kernels_gpu.test_paged_attention_decode_fused_rope compare the whole cache).

For "equals rope_cache_append" to be a statement about the append and not about two kernels' FMA
contraction, the rotation is exact in every form: qkv elements are multiples of 1/16 below 16 in
magnitude (in the slab forms x in {-2..2} times a sparse w in {-1, 0, 1} / 16 over K = 4096, so that
every slab slice and the sum are exact too) and the cos / sin table holds multiples of 1/4 in
[-1, 1]; a c - b s is then a multiple of 1/64 below 32, exact in fp32 however it is contracted."""
import functools
import math

import pytest
import torch

from distributed_llms_amd import _ext, ops
from distributed_llms_amd.ops import attention, gemm
from distributed_llms_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

HQ, HKV, D, BS, HIDDEN = 8, 2, 128, 32, 4096
SCALE = 1 / math.sqrt(D)
POISON = 1.0e30            # finite in bf16; 128 products with |q| < 16 stay finite in fp32
BATCHES = [(1, 2, 8), (9, 31, 32), (33, 40, 63), (64, 65, 97), (97, 1, 33)]
FORMS = ["bf16", "slab3", "slab5", "unfused"]
SPLITS = ["one", "own", "plan"]
BF16 = torch.bfloat16
POISON_BF16 = float(torch.tensor(POISON, dtype=BF16))


def _sixteenths(g, *shape, lim=32):
    return (torch.randint(-lim, lim + 1, shape, generator=g).float() / 16).to(BF16)


@functools.lru_cache(maxsize=None)
def _case(lens, fused):
    """Inputs of one batch, built once on the CPU and shared by every form / split of it: the block
    table, the admissible keys' K / V (key order), the poison-tail and zero-tail caches, q or x / w."""
    g = torch.Generator().manual_seed(1000 * sum(lens) + len(lens) + fused)
    b = len(lens)
    nblocks = [(n + BS - 1) // BS for n in lens]
    mb = max(nblocks)
    nb = 1 + sum(nblocks) + 2                                  # block 0 and two more: owned by nobody
    perm = (1 + torch.randperm(nb - 1, generator=g)).tolist()
    bt = torch.zeros(b, mb, dtype=torch.int32)
    i = 0
    for s, n in enumerate(nblocks):
        bt[s, :n] = torch.tensor(perm[i:i + n], dtype=torch.int32)
        i += n
    krow = ref._krow32()
    caches = {}
    data = [(_sixteenths(g, n - fused, HKV, D), _sixteenths(g, n - fused, HKV, D)) for n in lens]
    for name, fill in (("poison", POISON), ("zero", 0.0)):
        k = torch.full((nb, HKV, BS, D), fill, dtype=BF16)
        v = torch.full((nb, HKV, D, BS), fill, dtype=BF16)
        vg = v.view(nb, HKV, 4, D, 8)
        for s, n in enumerate(lens):
            for j in range(n - fused):                         # fused: key n - 1 is not in the cache yet
                blk, off = int(bt[s, j // BS]), j % BS
                k[blk, :, krow[off], :] = data[s][0][j]
                vg[blk, :, off // 8, :, off % 8] = data[s][1][j]
        caches[name] = (k.cuda(), v.cuda())
    c = dict(bt=bt.cuda(), sl=torch.tensor(lens, dtype=torch.int32).cuda(), mb=mb, caches=caches)
    if fused:
        c["pos"] = c["sl"] - 1
        c["slots"] = torch.tensor([int(bt[s, (n - 1) // BS]) * BS + (n - 1) % BS for s, n in enumerate(lens)],
                                  dtype=torch.int32).cuda()
        c["cs"] = (torch.randint(-4, 5, (128, D), generator=g).float() / 4).cuda()
        c["qkv"] = _sixteenths(g, b, (HQ + 2 * HKV) * D).cuda()
        c["x"] = torch.randint(-2, 3, (b, HIDDEN), generator=g).to(BF16).cuda()
        w = torch.randint(-1, 2, ((HQ + 2 * HKV) * D, HIDDEN), generator=g).float() / 16
        c["w"] = (w * (torch.rand(w.shape, generator=g) < 1 / 16)).to(BF16).cuda()
    else:
        c["q"] = _sixteenths(g, b, HQ, D).cuda()
    return c


def _split_plan(kind, mb):
    if kind == "one":
        return 1, mb * BS
    if kind == "own":
        return mb, BS                                          # every chunk, the tail too, in a split of its own
    return attention.decode_split_plan(len(BATCHES[0]), HKV, mb * BS, BS, mb)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(c, form, kind, k, v, part=None, qkv=None):
    """The native launchers with an explicit (splits, split_len), as ops.attention._decode calls them."""
    b = c["sl"].numel()
    splits, split_len = _split_plan(kind, c["mb"])
    out = torch.empty(b, HQ, D, dtype=BF16, device="cuda")
    po, pml = attention.decode_workspace(b, HQ, D, out.device, splits) if splits > 1 else (None, None)
    tail = (c["bt"].data_ptr(), c["sl"].data_ptr(), po.data_ptr() if splits > 1 else 0,
            pml.data_ptr() if splits > 1 else 0, b, HQ, HKV, D, BS, c["mb"], splits, split_len, float(SCALE))
    kern = _ext.kernels()
    if form == "unfused":
        kern.paged_attention_decode(out.data_ptr(), c["q"].data_ptr(), k.data_ptr(), v.data_ptr(), *tail, _stream())
    else:
        kern.paged_attention_decode_rope(
            out.data_ptr(), 0 if part is not None else qkv.data_ptr(), c["pos"].data_ptr(), c["cs"].data_ptr(),
            c["slots"].data_ptr(), k.data_ptr(), v.data_ptr(), *tail, 0 if part is None else part.ws.data_ptr(),
            0 if part is None else part.splits, 0 if part is None else part.m * part.n, _stream())
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("kind", SPLITS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("lens", BATCHES, ids=lambda t: "-".join(map(str, t)))
def test_tail_block(cuda, lens, form, kind):
    fused = form != "unfused"
    c = _case(lens, int(fused))
    part = qkv = None
    if form.startswith("slab"):
        part = gemm.linear_wide(c["x"], c["w"], splits=int(form[4:]), defer=True)
        assert isinstance(part, gemm.SplitKPartial) and part.splits == int(form[4:])
        qkv = part.materialize()                               # bf16 of the same sums (reads the slabs only)
        assert float(qkv.float().abs().max()) < 16 and torch.equal(qkv.float() * 16, (qkv.float() * 16).round())
    elif fused:
        qkv = c["qkv"]
    outs, after = {}, {}
    for name in ("poison", "zero"):
        k, v = (t.clone() for t in c["caches"][name])
        outs[name] = _launch(c, form, kind, k, v, part, qkv)
        after[name] = (k, v)
    # the fp32 reference over the admissible keys: the zero-tail cache, plus the new key when fused
    k2, v2 = (t.float() for t in c["caches"]["zero"])
    if fused:
        q2 = ref.rope_cache_append(qkv.float(), c["pos"], c["cs"], k2, v2, c["slots"], HQ, HKV, D)
    else:
        q2 = c["q"].float()
    expect = ref.paged_attention_decode(q2, k2, v2, c["bt"], c["sl"], SCALE)
    torch.testing.assert_close(outs["poison"].float(), expect, atol=2e-2, rtol=2e-2)
    assert torch.equal(_bits(outs["poison"]), _bits(outs["zero"])), "poison tail and zero tail: different output bits"
    for name in ("poison", "zero"):
        ke, ve = (t.clone() for t in c["caches"][name])
        if fused:
            ops.rope_cache_append(qkv, c["pos"], c["cs"], ke, ve, c["slots"], HQ, HKV, D, write_q=False)
        k, v, ke, ve = (t.cpu() for t in (*after[name], ke, ve))
        krow, bt, vg, vge = ref._krow32(), c["bt"].cpu(), v.view(-1, HKV, 4, D, 8), ve.view(-1, HKV, 4, D, 8)
        for s, n in enumerate(lens):
            for j in range(n):                                 # earlier keys unchanged; fused: key n - 1 appended
                blk, off = int(bt[s, j // BS]), j % BS
                assert torch.equal(_bits(k[blk, :, krow[off]]), _bits(ke[blk, :, krow[off]])), (name, "K", s, j)
                assert torch.equal(_bits(vg[blk, :, off // 8, :, off % 8]),
                                   _bits(vge[blk, :, off // 8, :, off % 8])), (name, "V", s, j)
        assert torch.equal(_bits(k), _bits(ke)) and torch.equal(_bits(v), _bits(ve)), (name, "stale slots")


def test_first_key_of_a_wholly_poisoned_block(cuda):
    """noff = 0, fused: at a context of 33 the new key's block holds nothing but poison, the kernel loads
    only the V^T group it writes back, the output is right and the new key lands in slot 0 of that block
    (K row krow32(0) = 0, element 0 of V^T group 0); the block's other slots keep the poison."""
    lens = (33, 33, 33)
    c = _case(lens, 1)
    k, v = (t.clone() for t in c["caches"]["poison"])
    out = ops.paged_attention_decode_rope(c["qkv"], c["pos"], c["cs"], k, v, c["slots"], c["bt"], c["sl"], HQ, HKV, D,
                                          SCALE)
    k2, v2 = (t.float() for t in c["caches"]["zero"])
    q2 = ref.rope_cache_append(c["qkv"].float(), c["pos"], c["cs"], k2, v2, c["slots"], HQ, HKV, D)
    expect = ref.paged_attention_decode(q2, k2, v2, c["bt"], c["sl"], SCALE)
    torch.testing.assert_close(out.float(), expect, atol=2e-2, rtol=2e-2)
    vg, v2g = v.view(-1, HKV, 4, D, 8), v2.view(-1, HKV, 4, D, 8)
    for s in range(len(lens)):
        blk = int(c["bt"][s, 1])
        assert int(c["slots"][s]) == blk * BS
        assert torch.equal(k[blk, :, 0].float(), k2[blk, :, 0]), ("K slot 0", s)
        assert torch.equal(vg[blk, :, 0, :, 0].float(), v2g[blk, :, 0, :, 0]), ("V slot 0", s)
        assert bool((k[blk, :, 1:].float() == POISON_BF16).all()), ("K poison", s)
        rest = vg[blk].float().clone()
        rest[:, 0, :, 0] = POISON_BF16
        assert bool((rest == POISON_BF16).all()), ("V poison", s)
