"""Sliding-window attention on the CPU: the masked reference against a dense fp64 softmax, config parsing,
the host-side refusals and plans, and tiny-mistral-sw against HF MistralForCausalLM."""
import math

import pytest
import torch
import transformers

from distributed_llms_amd import ops
from distributed_llms_amd.config import EngineConfig, ModelConfig, get_model_config
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.ops import reference as ref

HQ, HKV, D = 4, 2, 16


def _paged(lens, seed=0):
    """Dense k, v [Hkv, n, D] per sequence, appended to a shuffled paged cache with the project's own append."""
    g = torch.Generator().manual_seed(seed)
    nblk = [-(-n // 32) for n in lens]
    kc, vc = torch.zeros(sum(nblk) + 2, HKV, 32, D), torch.zeros(sum(nblk) + 2, HKV, D, 32)
    perm = torch.randperm(sum(nblk) + 2, generator=g).tolist()
    bt = torch.zeros(len(lens), max(nblk), dtype=torch.int32)
    dense = []
    for i, n in enumerate(lens):
        bt[i, :nblk[i]] = torch.tensor(perm[:nblk[i]])
        perm = perm[nblk[i]:]
        qkv = torch.randn(n, (HQ + 2 * HKV) * D, generator=g)
        slots = (bt[i, torch.arange(n) // 32] * 32 + torch.arange(n) % 32).to(torch.int32)
        ref.rope_cache_append(qkv, torch.arange(n, dtype=torch.int32), None, kc, vc, slots, HQ, HKV, D)
        k, v = qkv[:, HQ * D:].view(n, 2, HKV, D).unbind(1)
        dense.append((k.transpose(0, 1).double(), v.transpose(0, 1).double()))
    return kc, vc, bt, dense


def _dense(q, k, v, qpos, window):
    """fp64 softmax over a dense mask: query at position p sees keys j with max(0, p - W + 1) <= j <= p."""
    n = k.shape[1]
    j = torch.arange(n).view(1, n)
    p = qpos.view(-1, 1)
    keep = (j <= p) & ((j > p - window) if window else torch.ones_like(j, dtype=torch.bool))
    qi = q.double().permute(1, 0, 2).reshape(HKV, HQ // HKV, len(qpos), D)
    s = torch.einsum("hgqd,hnd->hgqn", qi, k) / math.sqrt(D)
    o = torch.einsum("hgqn,hnd->hgqd", torch.softmax(s.masked_fill(~keep, float("-inf")), -1), v)
    return o.reshape(HQ, len(qpos), D).permute(1, 0, 2)


@pytest.mark.parametrize("window", [1, 32, 33, 48])
def test_reference_against_dense_mask(window):
    """Decode and prefill (fresh, and chunked q_len < ctx) over contexts on both sides of W."""
    lens = [max(1, window - 1), window, window + 1, 3 * window + 5]
    kc, vc, bt, dense = _paged(lens, seed=window)
    sl = torch.tensor(lens, dtype=torch.int32)
    q = torch.randn(len(lens), HQ, D, generator=torch.Generator().manual_seed(1))
    got = ops.paged_attention_decode(q, kc, vc, bt, sl, 1 / math.sqrt(D), window=window)
    for i, n in enumerate(lens):
        want = _dense(q[i:i + 1], *dense[i], torch.tensor([n - 1]), window)
        torch.testing.assert_close(got[i:i + 1].double(), want, atol=1e-5, rtol=1e-5)
    for qlens in (lens, [min(n, 1 + i * 3) for i, n in enumerate(lens)]):
        cu = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0)), dtype=torch.int32)
        q = torch.randn(sum(qlens), HQ, D, generator=torch.Generator().manual_seed(2))
        got = ops.paged_attention_prefill(q, kc, vc, bt, cu, sl, 1 / math.sqrt(D), window=window)
        for i, (n, ql) in enumerate(zip(lens, qlens)):
            rows = slice(int(cu[i]), int(cu[i + 1]))
            want = _dense(q[rows], *dense[i], torch.arange(n - ql, n), window)
            torch.testing.assert_close(got[rows].double(), want, atol=1e-5, rtol=1e-5)


def test_window_that_covers_the_context_is_no_window():
    lens = [5, 70]
    kc, vc, bt, _ = _paged(lens)
    sl, cu = torch.tensor(lens, dtype=torch.int32), torch.tensor([0, 5, 75], dtype=torch.int32)
    q, qd = torch.randn(75, HQ, D), torch.randn(2, HQ, D)
    for w in (70, 1000):
        assert torch.equal(ref.paged_attention_prefill(q, kc, vc, bt, cu, sl, 0.25, w),
                           ref.paged_attention_prefill(q, kc, vc, bt, cu, sl, 0.25))
        assert torch.equal(ref.paged_attention_decode(qd, kc, vc, bt, sl, 0.25, w),
                           ref.paged_attention_decode(qd, kc, vc, bt, sl, 0.25, 0))


@pytest.mark.parametrize("sw,want", [(4096, 4096), (None, 0)])
def test_config_reads_and_writes_the_window(sw, want):
    hf = dict(get_model_config("mistral-7b").to_hf_config(), sliding_window=sw)
    assert hf["model_type"] == "mistral"
    cfg = ModelConfig.from_hf_config(hf)
    assert cfg.sliding_window == want and cfg.arch == "llama"
    back = cfg.to_hf_config()
    assert back.get("sliding_window", 0) == want
    assert ModelConfig.from_hf_config(back).sliding_window == want
    assert ModelConfig.from_hf_config(dict(hf, model_type="llama")).sliding_window == 0
    assert get_model_config("mistral-7b").sliding_window == 4096
    assert get_model_config("tiny-llama").sliding_window == 0


def test_host_refusals_route_and_plan():
    x = torch.zeros(1, (HQ + 2 * HKV) * D)
    with pytest.raises(ValueError, match="sliding-window"):
        ops.paged_attention_decode_rope(x, None, None, None, None, None, None, None, HQ, HKV, D, 1.0, window=4)
    with pytest.raises(ValueError, match="sliding-window"):
        ops.paged_attention_prefill_rope(x, None, None, None, None, None, None, None, HQ, D, 1.0, window=4)
    # the route: its own version over a rotated q, whatever the shapes -- also behind tables wider than 32k tokens
    for args in ((1, 32, 8, 128, 16384, 16384, 512), (8, 32, 8, 128, 5, 40000, 1250)):
        r = ops.prefill_route(*args, window=4096)
        assert r == ops.PrefillRoute(ops.PREFILL_WINDOW, False) and r.version not in (5, 7, 9)
    with pytest.raises(ValueError, match="block ids"):
        ops.prefill_route(1, 32, 8, 128, 64, 64, 2, window=ops.prefill_window_max(4) + 1)
    # the decode plan: no context argument, covers ceil(W / 32) + 1 blocks, same plan inside a batch bucket
    for b, w in ((1, 1), (3, 96), (64, 4096), (256, 4096)):
        n, sb = ops.decode_window_plan(b, 8, w)
        assert n * sb >= -(-w // 32) + 1 and (n - 1) * sb < -(-w // 32) + 1 and 1 <= n <= ops.MAX_DECODE_SPLITS
    assert ops.decode_window_plan(5, 8, 4096) == ops.decode_window_plan(8, 8, 4096)


def test_tiny_mistral_matches_transformers():
    """The same weights in HF MistralForCausalLM (eager attention, fp32): the last-token logits of a prompt
    of 3 W tokens, and ten greedy tokens decoded past it (tolerance of tests/test_model_vs_hf.py)."""
    name = "tiny-mistral-sw"
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=11, dtype=torch.float32)
    hfc = {k: v for k, v in cfg.to_hf_config().items()
           if not k.startswith("_") and k not in ("architectures", "model_type")}
    assert hfc["sliding_window"] == 48
    m = transformers.MistralForCausalLM(transformers.MistralConfig(**hfc, attn_implementation="eager"))
    missing, _ = m.load_state_dict(sd, strict=False)
    assert not missing, missing
    m.eval()
    stage = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)
    assert stage.window == 48
    eng = LLMEngine(EngineConfig(model=name, dtype="float32", device="cpu", max_batch=4, max_seq_len=256,
                                 use_graphs=False), stage)
    prompt = torch.randint(3, cfg.vocab_size, (3 * 48,), generator=torch.Generator().manual_seed(5)).tolist()
    eng.add_request(prompt, SamplingParams(max_new_tokens=1))
    logits = eng.runner.execute(build_host_batch(eng.scheduler.schedule(0), eng.bm, 32))
    with torch.no_grad():
        want = m(torch.tensor([prompt])).logits[0, -1]
        full = transformers.MistralForCausalLM(transformers.MistralConfig(**dict(hfc, sliding_window=None),
                                                                          attn_implementation="eager"))
        full.load_state_dict(sd, strict=False)
        assert (full.eval()(torch.tensor([prompt])).logits[0, -1] - want).abs().max() > 1e-3   # the window matters
    torch.testing.assert_close(logits[0], want, atol=1e-4, rtol=1e-4)
    eng2 = LLMEngine(EngineConfig(model=name, dtype="float32", device="cpu", max_batch=4, max_seq_len=256,
                                  use_graphs=False), stage)
    out = eng2.generate([prompt], SamplingParams(max_new_tokens=10, ignore_eos=True))[0]
    with torch.no_grad():
        g = m.generate(torch.tensor([prompt]), max_new_tokens=10, min_new_tokens=10, do_sample=False, pad_token_id=0)
    assert g[0, len(prompt):].tolist() == out
