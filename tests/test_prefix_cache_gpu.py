"""Prefix caching on the GPU (tiny-llama-d128, a small KV pool): the tail prefill of a request whose
header is in the paged cache against the CPU fp32 whole-prompt prefill, with the default attention
choice and with the split-context kernel forced; a mixed workload with graphs and lookahead, cache on
against off; a 2-stage pipeline of stage threads with the cache on."""
import gc

import numpy as np
import pytest
import torch

from distributed_llms_amd import knobs, ops
from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.ops import attention

pytestmark = pytest.mark.gpu
NAME = "tiny-llama-d128"


@pytest.mark.parametrize("attn", [0, ops.PREFILL_SPLIT], ids=["default", "split"])
def test_tail_prefill_after_a_hit_matches_cpu_logits(cuda, attn):
    """A second request sharing a 300-token header with a finished first one prefills 32 tokens over
    288 cached ones; its logits against the CPU fp32 prefill of the whole prompt, at the rule of
    test_chunked_prefill_gpu_matches_cpu_logits."""
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    header = [(13 * j) % 400 + 3 for j in range(300)]
    first, second = header + [7, 8, 9], header + [(29 * j) % 300 + 5 for j in range(20)]
    e_cpu = LLMEngine(EngineConfig(model=NAME, dtype="float32", device="cpu", max_batch=2, max_seq_len=512,
                                   use_graphs=False),
                      ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd))
    e_gpu = LLMEngine(EngineConfig(model=NAME, dtype="bfloat16", device="cuda", max_batch=2, max_seq_len=512,
                                   use_graphs=False, num_kv_blocks=32, enable_prefix_caching=True),
                      ModelStage(cfg, 0, cfg.num_layers, "cuda", torch.bfloat16).load_hf_state(sd))
    with knobs.override(prefill_attn=attn):
        e_gpu.generate([first], SamplingParams(max_new_tokens=2, ignore_eos=True))
        assert e_gpu.bm.num_registered() == 9 and e_gpu.bm.num_evictable() == 9
        logits = []
        for eng in (e_cpu, e_gpu):
            seq = eng.add_request(second, SamplingParams(max_new_tokens=1))
            st = eng.scheduler.schedule(0)
            hb = build_host_batch(st, eng.bm, 32)
            logits.append(eng.runner.execute(hb).float().cpu())
        assert seq.cached_tokens == 288 and hb.num_tokens == 32 and int(hb.positions[0]) == 288
        assert ops.prefill_route(1, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, hb.num_tokens, None,
                                 hb.block_tables.shape[1]).rope_in_kernel == (attn == 0)
    torch.testing.assert_close(logits[1], logits[0], atol=6e-2, rtol=5e-2)


def _hit_engines(num_kv_blocks=64):
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    e_cpu = LLMEngine(EngineConfig(model=NAME, dtype="float32", device="cpu", max_batch=4, max_seq_len=1024,
                                   use_graphs=False),
                      ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd))
    e_gpu = LLMEngine(EngineConfig(model=NAME, dtype="bfloat16", device="cuda", max_batch=4, max_seq_len=1024,
                                   use_graphs=False, num_kv_blocks=num_kv_blocks, enable_prefix_caching=True),
                      ModelStage(cfg, 0, cfg.num_layers, "cuda", torch.bfloat16).load_hf_state(sd))
    return cfg, e_cpu, e_gpu


def _count_attention_paths(monkeypatch):
    """Counters of the calls that reach the split kernel, the in-kernel-RoPE prefill and the
    rotated-q append, as the stage makes them."""
    n = {"split": 0, "rope_attn": 0, "write_q": 0}
    split, rope_attn, append = attention._prefill_split, ops.paged_attention_prefill_rope, ops.rope_cache_append

    def count(key, fn, when=lambda a, k: True):
        def wrapped(*a, **k):
            n[key] += bool(when(a, k))
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(attention, "_prefill_split", count("split", split))
    monkeypatch.setattr(ops, "paged_attention_prefill_rope", count("rope_attn", rope_attn))
    monkeypatch.setattr(ops, "rope_cache_append", count("write_q", append, lambda a, k: k.get("write_q", True)))
    return n


# 600 + 20 tokens: a hit of 18 blocks (576 tokens), a 44-token tail over 620 tokens of context = 20 chunks,
# the shortest the split plan's floor of 8 chunks per split divides in two
HEADER = [(13 * j) % 400 + 3 for j in range(600)]
SECOND = HEADER + [(29 * j) % 300 + 5 for j in range(20)]
HIT, TAIL = 576, 44


def test_default_dispatch_takes_the_split_kernel_after_a_hit(cuda, monkeypatch):
    """The engine's own route: no kernel forced, the cutover knob lowered to this test's context.  The
    tail step of a hit must go through prefill_split_eligible, the rotated-q append and the split
    kernel in every layer (a dropped max_ctx or a wrong shape tuple in the stage would leave it on v4),
    and meet the logits rule; with the knob at its default the same step stays on the in-kernel-RoPE path."""
    cfg, e_cpu, e_gpu = _hit_engines()
    e_gpu.generate([HEADER + [7, 8, 9]], SamplingParams(max_new_tokens=2, ignore_eos=True))
    e_cpu.add_request(SECOND, SamplingParams(max_new_tokens=1))
    want = e_cpu.runner.execute(build_host_batch(e_cpu.scheduler.schedule(0), e_cpu.bm, 32)).float()
    seq = e_gpu.add_request(SECOND, SamplingParams(max_new_tokens=1))
    st = e_gpu.scheduler.schedule(0)
    hb = build_host_batch(st, e_gpu.bm, 32)
    assert seq.cached_tokens == HIT and hb.num_tokens == TAIL and hb.max_ctx == 620 and not st.mixed
    assert knobs.K.prefill_attn == 0
    with knobs.override(prefill_split_min_ctx=256):
        assert ops.prefill_split_eligible(1, cfg.num_kv_heads, TAIL, 620, cfg.num_heads // cfg.num_kv_heads)
    n = _count_attention_paths(monkeypatch)
    plain = e_gpu.runner.execute(hb).float().cpu()
    assert n == {"split": 0, "rope_attn": cfg.num_layers, "write_q": 0}         # 620 < 4096: as the parent runs it
    with knobs.override(prefill_split_min_ctx=256):
        got = e_gpu.runner.execute(hb).float().cpu()                            # the same step again: same cache writes
    assert n == {"split": cfg.num_layers, "rope_attn": cfg.num_layers, "write_q": cfg.num_layers}
    torch.testing.assert_close(got, want, atol=6e-2, rtol=5e-2)
    torch.testing.assert_close(plain, want, atol=6e-2, rtol=5e-2)


def test_mixed_step_takes_the_split_kernel_after_a_hit(cuda, monkeypatch):
    """A late request whose slot is decoding is admitted into a MIXED step (the common serving case):
    its tail rows reach the split kernel by default too, the decode rows keep the decode kernel."""
    cfg, e_cpu, e_gpu = _hit_engines()
    e_gpu.generate([HEADER + [7, 8, 9]], SamplingParams(max_new_tokens=2, ignore_eos=True))
    e_cpu.add_request(SECOND, SamplingParams(max_new_tokens=1))
    want = e_cpu.runner.execute(build_host_batch(e_cpu.scheduler.schedule(0), e_cpu.bm, 32)).float()
    e_gpu.add_request([5, 6, 7, 8, 9], SamplingParams(max_new_tokens=50, ignore_eos=True))
    for _ in range(3):                      # its prefill, then two decode steps: the slot is running
        st = e_gpu.scheduler.schedule(0)
        e_gpu.scheduler.complete(st, e_gpu.execute_step(st))
    assert e_gpu.scheduler.num_running() == 1
    seq = e_gpu.add_request(SECOND, SamplingParams(max_new_tokens=1))
    st = e_gpu.scheduler.schedule(0)
    assert st.mixed and st.num_decode == 1 and st.seqs == [seq] and seq.cached_tokens == HIT
    hb = e_gpu._host_batch(st)
    assert hb.num_decode == 1 and hb.num_tokens == 1 + TAIL
    n = _count_attention_paths(monkeypatch)
    with knobs.override(prefill_split_min_ctx=256):
        got = e_gpu.runner.execute(hb).float().cpu()
    assert n["split"] == cfg.num_layers and n["rope_attn"] == 0
    torch.testing.assert_close(got[-1:], want, atol=6e-2, rtol=5e-2)


def test_mixed_workload_cache_on_vs_off(cuda):
    """Shared headers arriving in waves during decode, graphs and lookahead on.  Batch composition
    changes the GEMMs' split-K counts (a hit shortens the prefill), so bf16 greedy outputs may part at
    near-ties: the share of exact sequences test_mixed_prefill_decode_steps_gpu demands (11 of 14),
    every sequence with the right length."""
    def run(cache):
        eng = LLMEngine(EngineConfig(model="synthetic:" + NAME, max_batch=16, max_seq_len=256, num_kv_blocks=96,
                                     mixed_prefill_tokens=64, graph_batch_sizes=(4, 8, 16),
                                     enable_prefix_caching=cache))
        assert eng.lookahead and eng.ecfg.use_graphs
        rng = np.random.default_rng(5)
        hdrs = [rng.integers(3, 500, size=n).tolist() for n in (70, 40)]
        prompts = [hdrs[i % 2] + rng.integers(3, 500, size=int(rng.integers(2, 30))).tolist() for i in range(14)]
        p = SamplingParams(max_new_tokens=12, ignore_eos=True)
        seqs, i, step = [], 0, 0
        waves = [(0, 4), (3, 4), (6, 3), (10, 3)]
        while waves or eng.has_work():
            while waves and waves[0][0] <= step:
                _, n = waves.pop(0)
                seqs += [eng.add_request(q, p) for q in prompts[i:i + n]]
                i += n
            eng.step()
            step += 1
        return [s.output for s in seqs], eng, seqs

    ref, e0, _ = run(False)
    out, e1, seqs = run(True)
    assert all(len(o) == 12 for o in out)
    assert sum(a == b for a, b in zip(out, ref)) >= 11, (out, ref)
    hits = e1.scheduler.prefix_stats()["hit_tokens"]
    assert hits > 0 and hits == sum(s.cached_tokens for s in seqs)
    assert e0.scheduler.prefix_stats()["hit_tokens"] == 0
    assert e1.num_lookahead > 0 and e1.bm.num_free() == 95 and not e1.scheduler._pending


def test_two_stage_pipeline_with_the_cache(cuda):
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=9, dtype=torch.float32)
    ecfg = EngineConfig(model=NAME, dtype="bfloat16", device="cuda", max_batch=4, max_seq_len=256,
                        num_kv_blocks=128, graph_batch_sizes=(1, 2, 4), enable_prefix_caching=True)
    header = [(7 * j) % 300 + 3 for j in range(70)]
    prompts = [header + [i + 1, 2 * i + 3, 5, 7, 11 + i] for i in range(10)]
    p = SamplingParams(max_new_tokens=12, ignore_eos=True)
    single = LLMEngine(ecfg, ModelStage(cfg, 0, cfg.num_layers, "cuda", torch.bfloat16).load_hf_state(sd))
    ref = single.generate(prompts, p)
    hits = single.scheduler.prefix_stats()["hit_tokens"]
    # the engine goes before the pipeline captures: its graphs were captured inside the runner's
    # inference mode, and while they live a capture outside it (the pipeline's warm-up) cannot
    # update the generator state they share
    del single
    gc.collect()
    outs, drv, _ = run_loopback_pipeline(ecfg, 2, prompts, p, device="cuda", hf_state=sd)
    assert outs == ref
    assert hits > 0 and drv.scheduler.prefix_stats()["hit_tokens"] > 0
