"""The sliding-window attention kernels (attention_swa.hip) against the fp32 reference (gfx950 only), at the
tolerance of the bf16 attention tests of tests/test_kernels_gpu.py.  Every case runs on a POISONED cache --
1e4 in every key and value outside a sequence's window and in every block no table names -- and is compared
with the reference on the clean cache: a key read from outside the window cannot hide."""
import math

import numpy as np
import pytest
import torch

import teacher_forced as tf
from distributed_llms_amd import ops
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TOL = dict(atol=2e-2, rtol=2e-2)
SHAPES = [(4, 4, 64), (8, 2, 128), (16, 2, 64), (8, 1, 128)]     # (hq, hkv, d): GQA groups 1, 4, 8, 8


def _caches(lens, qlens, window, hkv, d, width=None, seed=0):
    """(clean k, v, poisoned k, v, block tables) for sequences of ``lens`` keys whose last ``qlens`` are queries."""
    g = torch.Generator().manual_seed(seed)
    nblk = [-(-n // 32) for n in lens]
    nb = sum(nblk) + 3
    k, v = torch.randn(nb, hkv, 32, d, generator=g).bfloat16(), torch.randn(nb, hkv, d, 32, generator=g).bfloat16()
    kp, vp = torch.full_like(k, 1e4), torch.full_like(v, 1e4)
    perm = torch.randperm(nb, generator=g).tolist()
    bt = torch.zeros(len(lens), width or max(nblk), dtype=torch.int32)
    v5, vp5 = v.view(nb, hkv, 4, d, 8), vp.view(nb, hkv, 4, d, 8)
    for i, (n, ql) in enumerate(zip(lens, qlens)):
        bt[i, :nblk[i]] = torch.tensor(perm[:nblk[i]])
        perm = perm[nblk[i]:]
        j = torch.arange(max(0, n - ql - window + 1), n)         # the keys some query of the sequence sees
        blk, row = bt[i, j // 32].long(), ref._KROW32[j % 32]
        kp[blk, :, row] = k[blk, :, row]
        vp5[blk, :, (j % 32) // 8, :, j % 8] = v5[blk, :, (j % 32) // 8, :, j % 8]
    return [x.cuda() for x in (k, v, kp, vp, bt)]


@pytest.mark.parametrize("window", [1, 32, 40, 96])
@pytest.mark.parametrize("hq,hkv,d", SHAPES)
def test_decode_window(cuda, hq, hkv, d, window):
    """Contexts W - 1, W, W + 1 and 3 W + 5 in one batch: the window starts at key 0, on a block edge, mid-block."""
    lens = [max(1, window - 1), window, window + 1, 3 * window + 5]
    k, v, kp, vp, bt = _caches(lens, [1] * 4, window, hkv, d, seed=window)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q = torch.randn(4, hq, d, device="cuda").bfloat16()
    out = ops.paged_attention_decode(q, kp, vp, bt, sl, 1 / math.sqrt(d), window=window)
    want = ref.paged_attention_decode(q.float(), k.float(), v.float(), bt, sl, 1 / math.sqrt(d), window)
    torch.testing.assert_close(out.float(), want, **TOL)


@pytest.mark.parametrize("hq,hkv,d,window", [(8, 2, 128, 96), (4, 4, 64, 40)])
def test_decode_window_bits_do_not_depend_on_the_batch_or_the_table(cuda, hq, hkv, d, window):
    lens = [3 * window + 5, window + 1, 7]
    k, v, kp, vp, bt = _caches(lens, [1] * 3, window, hkv, d)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q = torch.randn(3, hq, d, device="cuda").bfloat16()
    run = lambda q, bt, sl, **kw: ops.paged_attention_decode(q, kp, vp, bt, sl, 0.1, window=window, **kw)
    base = run(q, bt, sl)
    assert torch.equal(base, run(q, bt, sl))
    wide = torch.cat([bt, torch.zeros_like(bt)], 1).contiguous()
    assert torch.equal(base, run(q, wide, sl, max_ctx=wide.shape[1] * 32))
    rep = lambda x: x.repeat(16, *[1] * (x.dim() - 1)).contiguous()
    assert torch.equal(rep(base), run(rep(q), rep(bt), rep(sl)))      # batch 48


@pytest.mark.parametrize("window", [1, 32, 40, 96])
@pytest.mark.parametrize("hq,hkv,d", SHAPES[:3])
def test_prefill_window(cuda, hq, hkv, d, window):
    """Fresh prompts of W - 1, W + 1 and 4 W + 7 tokens; tails of 1, 5 and 40 rows over 5 W keys; one sequence
    behind a table of 1,100 blocks (wider than the causal LDS kernels stage)."""
    fresh = [max(1, window - 1), window + 1, 4 * window + 7]
    tails = [min(t, 5 * window) for t in (1, 5, 40)]
    for lens, qlens, width in ((fresh, fresh, None), ([5 * window] * 3, tails, None), ([5 * window], [5], 1100)):
        k, v, kp, vp, bt = _caches(lens, qlens, window, hkv, d, width=width, seed=window)
        sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        cu = torch.tensor([0] + np.cumsum(qlens).tolist(), dtype=torch.int32, device="cuda")
        q = torch.randn(sum(qlens), hq, d, device="cuda").bfloat16()
        out = ops.paged_attention_prefill(q, kp, vp, bt, cu, sl, 1 / math.sqrt(d), max_q_len=max(qlens), window=window)
        assert torch.equal(out, ops.paged_attention_prefill(q, kp, vp, bt, cu, sl, 1 / math.sqrt(d), window=window))
        want = ref.paged_attention_prefill(q.float(), k.float(), v.float(), bt, cu, sl, 1 / math.sqrt(d), window)
        torch.testing.assert_close(out.float(), want, **TOL)


def _reference_logits(name, sd, seqs):
    """{seq_id: (logits of every position, margins)} from the CPU fp32 stage holding the bf16-rounded weights:
    each sequence's prompt + output in one windowed prefill whose every row yields logits."""
    eng = tf.make_engine(name, {k: t.bfloat16().float() for k, t in sd.items()}, "cpu", max_prefill_tokens=1024)
    out = {}
    for s in seqs:
        eng.add_request(list(s.prompt) + list(s.output), tf.greedy(1))
        hb = build_host_batch(eng.scheduler.schedule(0), eng.bm, 32)
        hb.logits_idx = np.arange(len(hb.ids), dtype=np.int32)
        lg = eng.runner.execute(hb).float()
        out[s.seq_id] = (lg, torch.ones(lg.shape[0]))
        while eng.has_work():
            eng.step()
    return out


def test_engine_tiny_mistral(cuda):
    """Greedy runs of 20 / 100 / 300-token prompts, chunked and mixed, decode graphs on and off: the same tokens,
    and every logits row within tiny-llama's bound (the same dimensions) of the windowed CPU fp32 stage."""
    name = "tiny-mistral-sw"
    cfg, sd = tf.state_dict(name, tf.SHARPEN["tiny-llama"])
    tokens = []
    for graphs in (True, False):
        eng = tf.make_engine(name, sd, "cuda", use_graphs=graphs, max_prefill_tokens=64, mixed_prefill_tokens=64)
        assert eng.stage.window == 48
        waves = [(0, [(p, 40) for p in tf.prompts_of([20, 300], cfg.vocab_size, seed=4)]),
                 (4, [(p, 40) for p in tf.prompts_of([100], cfg.vocab_size, seed=9)])]
        seqs, rec = tf._drive(eng, None, waves)
        assert rec.num_chunk_rows > 1 and eng.scheduler.num_mixed > 0
        assert (eng.runner.graphs is not None and bool(eng.runner.graphs.num_replays)) == graphs
        tokens.append([list(s.output) for s in seqs])
        tf.compare(rec.records, _reference_logits(name, sd, seqs), tf.GPU_BOUNDS["tiny-llama"], seqs,
                   what=f"{name} graphs={graphs}")
    assert tokens[0] == tokens[1] and all(len(o) == 40 for o in tokens[0])
