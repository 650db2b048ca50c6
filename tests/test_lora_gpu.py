"""The multi-LoRA kernels (csrc/kernels/lora.hip) and the engine path on the GPU.

Kernel tests: bit-exact against fp64 on integer data (preconditions: tests/lora_cases.py, checked
on the CPU in tests/test_lora.py), a needle test, and random bf16 inputs against the fp64
evaluation of the contract within a derived per-element bound (lora_cases.random_case).  Every run
has guard rows and guard columns around y (they must keep their bits) and a NaN-filled workspace
(a partial read before it is written poisons the result).
"""
import numpy as np
import pytest
import torch

import lora_cases as lc
from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.ops import lora as lo

pytestmark = pytest.mark.gpu

GUARD = 16                   # guard columns right of y (a multiple of 4 keeps the rows 8-byte aligned)
SENTINEL = -777.0            # exact in bf16


def _run(c, dev="cuda"):
    """shrink + expand on the case; returns (y [T, N] on the host, the padded buffer on the host)."""
    t, n = c.y0.shape
    k = c.x.shape[1]
    buf = torch.full((t + 2, n + GUARD), SENTINEL, dtype=torch.bfloat16, device=dev)
    y = buf[1:t + 1, :n]
    y.copy_(c.y0.to(dev))
    w = lo.LoraWeight(c.a.to(dev), c.b.to(dev), c.scale.to(dev), c.starts)
    plan = lo.make_plan(c.slot.numpy(), dev)
    assert plan.nt <= lo.max_tiles(t, lc.NSLOTS)
    ws = torch.full((lo.workspace_floats(k, plan.nt, w.a.shape[1]),), float("nan"), dtype=torch.float32, device=dev)
    lo.expand(y, lo.shrink(c.x.to(dev), w, plan, ws), k, w, plan)
    torch.cuda.synchronize()
    return y.cpu(), buf.cpu()


def _check_guards(buf, t, n):
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[t + 1] == SENTINEL).all()), "guard rows written"
    assert bool((buf[:, n:] == SENTINEL).all()), "guard columns written"


EXACT = [(t, k, r, w) for t in (1, 15, 17, 33) for k, r, w in
         ((256, 1, (256, 128, 128)), (4096, 8, (256, 128, 48)), (256, 16, (272,)), (4096, 64, (256, 128, 128)))]


@pytest.mark.parametrize("t,k,rank,widths", EXACT)
def test_exact_integer_cases(cuda, t, k, rank, widths):
    c = lc.int_case(t, k, rank, widths)
    y, buf = _run(c)
    _check_guards(buf, t, sum(widths))
    assert torch.equal(y[c.slot < 0], c.y0[c.slot < 0]), "a row without an adapter was touched"
    assert torch.equal(y, c.expected), f"{(y != c.expected).sum().item()} of {y.numel()} elements differ"


def test_needle(cuda):
    t, n = 33, 272
    c = lc.needle_case(t, 4096, 8, n)
    y, buf = _run(c)
    _check_guards(buf, t, n)
    changed = y != c.y0
    for r in range(t):
        s = int(c.slot[r])
        cols = changed[r].nonzero().flatten().tolist()
        assert cols == ([] if s < 0 else [int(c.rounded[s])]), (r, s, cols)
    assert bool(((y.double() - c.expected).abs() <= c.ties).all())


@pytest.mark.parametrize("t,k,rank,widths", [(33, 4096, 64, (256, 128, 128)), (17, 256, 8, (256, 128, 48)),
                                             (300, 4096, 16, (4096,))])
def test_random_inputs_within_derived_bound_and_deterministic(cuda, t, k, rank, widths):
    c = lc.random_case(t, k, rank, widths)
    y, buf = _run(c)
    _check_guards(buf, t, sum(widths))
    assert bool(torch.isfinite(y.float()).all())
    err = (y.double() - c.expected).abs()
    bad = err > c.rounded
    assert not bool(bad.any()), f"{bad.sum().item()} elements above the bound, worst ratio " \
                                f"{(err / c.rounded.clamp(min=1e-300))[bad].max().item():.3f}"
    assert torch.equal(y[c.slot < 0], c.y0[c.slot < 0])
    y2, _ = _run(c)
    assert torch.equal(y, y2), "two runs must be bit-equal"


def test_padded_plan_tiles_are_inert(cuda):
    """A graph's static plan: unused tiles (slot -1) and a stale, larger plan do nothing."""
    c = lc.int_case(17, 256, 8, (256, 128, 48))
    dev = "cuda"
    t, n = c.y0.shape
    w = lo.LoraWeight(c.a.to(dev), c.b.to(dev), c.scale.to(dev), c.starts)
    nt = lo.max_tiles(t, lc.NSLOTS) + 3
    ts, tr = lo.row_plan(c.slot.numpy(), nt)
    plan = lo.LoraPlan(c.slot.to(dev), torch.from_numpy(ts).to(dev), torch.from_numpy(tr).to(dev), nt)
    y = c.y0.to(dev).clone()
    lo.apply(y, c.x.to(dev), w, plan)
    assert torch.equal(y.cpu(), c.expected)


# ------------------------------------------------------------------ engine
ADAPTERS = {"alpha": "synthetic:8:11", "beta": "synthetic:16:12:q_proj+v_proj+down_proj"}
ATTN_ONLY = {"alpha": "synthetic:8:11:q_proj+k_proj+v_proj+o_proj", "beta": "synthetic:4:12:q_proj+o_proj"}
PROMPTS = [[1, 5, 9, 200, 37, 44, 45, 46, 47, 48], [3, 4], list(range(10, 80)), [8] * 33, [9, 9, 9]]
WHO = [None, "alpha", "beta", "alpha", None]


def _gpu_engine(name, adapters, graphs=False, **kw):
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    args = dict(model=name, dtype="bfloat16", device="cuda", max_batch=8, max_seq_len=512, use_graphs=graphs,
                num_kv_blocks=256, graph_batch_sizes=(1, 2, 4, 8), lora_modules=dict(adapters or {}))
    args.update(kw)
    return LLMEngine(EngineConfig(**args), ModelStage(cfg, 0, cfg.num_layers, "cuda", torch.bfloat16).load_hf_state(sd))


def _cpu_engine(name, adapters):
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    return LLMEngine(EngineConfig(model=name, dtype="float32", device="cpu", max_batch=8, max_seq_len=512,
                                  use_graphs=False, lora_modules=dict(adapters)),
                     ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd))


def _params(who, n=16):
    return SamplingParams(max_new_tokens=n, ignore_eos=True, adapter=who)


@pytest.mark.parametrize("name,adapters", [("tiny-llama", ADAPTERS), ("tiny-llama-d128", ADAPTERS),
                                           ("tiny-mixtral", ATTN_ONLY)])
def test_prefill_logits_gpu_vs_cpu_with_adapters(cuda, name, adapters):
    outs = []
    for eng in (_cpu_engine(name, adapters), _gpu_engine(name, adapters)):
        for p, w in zip(PROMPTS, WHO):
            eng.add_request(p, SamplingParams(max_new_tokens=1, adapter=w))
        hb = build_host_batch(eng.scheduler.schedule(0), eng.bm, 32)
        assert hb.lora is not None
        outs.append(eng.runner.execute(hb).float().cpu())
    torch.testing.assert_close(outs[1], outs[0], atol=5e-2, rtol=5e-2)
    # and the adapters are not a no-op at that tolerance: the base model's logits are further away
    base = _cpu_engine(name, adapters)
    for p in PROMPTS:
        base.add_request(p, SamplingParams(max_new_tokens=1))
    lb = base.runner.execute(build_host_batch(base.scheduler.schedule(0), base.bm, 32)).float()
    assert (lb[1:4] - outs[0][1:4]).abs().max().item() > 0.2


def test_graphs_match_eager_on_a_mixed_adapter_batch(cuda):
    plist = [_params(w) for w in WHO]
    a = _gpu_engine("tiny-llama", ADAPTERS, graphs=False).generate(PROMPTS, plist)
    eng = _gpu_engine("tiny-llama", ADAPTERS, graphs=True)
    b = eng.generate(PROMPTS, plist)
    assert a == b
    gr = eng.runner.graphs
    keys = [k for k in gr.graphs if k[2]]
    assert keys and sum(gr.num_replays.get(k, 0) for k in keys) >= 10, "no (..., True) graph captured and replayed"


def test_lookahead_on_matches_off(cuda):
    plist = [_params(w) for w in WHO]
    on = _gpu_engine("tiny-llama", ADAPTERS, graphs=True)
    off = _gpu_engine("tiny-llama", ADAPTERS, graphs=True, kernel_knobs={"lookahead": False})
    assert on.lookahead and not off.lookahead
    a, b = on.generate(PROMPTS, plist), off.generate(PROMPTS, plist)
    assert a == b and on.num_lookahead > 0


def test_two_stage_pipeline_matches_single_engine(cuda):
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    plist = [_params(w, 8) for w in WHO]
    ecfg = EngineConfig(model="synthetic:tiny-llama", dtype="bfloat16", device="cuda", max_batch=8, max_seq_len=256,
                        num_kv_blocks=128, graph_batch_sizes=(1, 2, 4, 8), lora_modules=dict(ADAPTERS))
    single = LLMEngine(ecfg).generate(PROMPTS, plist)
    outs = run_loopback_pipeline(ecfg, 2, PROMPTS, plist, device="cuda")
    outs = outs[0] if isinstance(outs, tuple) else outs
    assert outs == single


def test_unused_adapters_leave_tokens_unchanged(cuda):
    p = _params(None)
    a = _gpu_engine("tiny-llama", ADAPTERS, graphs=True).generate(PROMPTS, p)
    b = _gpu_engine("tiny-llama", None, graphs=True).generate(PROMPTS, p)
    assert a == b
