"""The fused LM-head log-likelihood kernel (ops.lm_head_logprobs) against a float64 log-softmax at the smallest
shapes at which it can go wrong, and the engine's prompt_logprobs against the float32 CPU engine.

Tolerance of the exact cases (not fitted to the kernel): the same formula in float32 torch on the CPU has a largest
error E against float64 on these inputs; the kernel splits its sum over up to 2 S partials with a rescale each, so it
gets 4 E, plus 2^-22 |lp| for the final subtraction.  Both figures are printed."""
import math

import pytest
import torch

from distributed_llms_amd import ops
from distributed_llms_amd.ops import gemm

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64


def targets_for(t, v):
    """Row i asks for column V - 1, column 0, a column of the ragged last tile, or nothing (-1)."""
    last = (v - 1) // 256 * 256
    return torch.tensor([(v - 1, 0, last + i * 7 % (v - last), -1)[i % 4] for i in range(t)], dtype=torch.int32)


def softmax_gather(z, tg, dtype):
    """(l_t - m) - ln(sum exp(l - m)) in ``dtype`` on logits ``z``; 0.0 where the target is negative."""
    z = z.to(dtype)
    d = z - z.max(dim=1, keepdim=True).values
    lp = d.gather(1, tg.clamp(min=0).long()[:, None])[:, 0] - d.exp().sum(dim=1).log()
    return torch.where(tg >= 0, lp, torch.zeros_like(lp)).to(F64)


def exact_bound(z, tg):
    """(float64 result, per-row bound 4 E + 2^-22 |lp|) for logits ``z`` that bf16 holds exactly."""
    want = softmax_gather(z, tg, F64)
    e = (softmax_gather(z, tg, torch.float32) - want).abs().max().item()
    print(f"float32 reference error E {e:.3e}, bound 4 E + 2^-22 |lp| <= {4 * e + 2.0 ** -22 * want.abs().max().item():.3e}")
    return want, 4 * e + 2.0 ** -22 * want.abs()


def run_twice(x, w, tg, dev, ranges):
    """The op on a NaN-filled workspace, twice: equal bits, the first result back on the CPU as float64."""
    gemm._workspace(torch.device(dev)).fill_(float("nan"))
    a, b = (ops.lm_head_logprobs(x.to(dev), w.to(dev), tg.to(dev), ranges) for _ in range(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return a.cpu().to(F64)


@pytest.mark.parametrize("ranges", [1, 0])
@pytest.mark.parametrize("k", [64, 448])
@pytest.mark.parametrize("v", [8, 777, 5003])
@pytest.mark.parametrize("t", [1, 255, 257])
def test_exact_operands(cuda, t, v, k, ranges):
    """x rows with eight +-1 entries, w in -3 .. 3: every dot product is an integer of at most 24, exact in f32 and
    in bf16, so the logits are known and only the softmax arithmetic is under test."""
    g = torch.Generator().manual_seed(t * 7 + v + k)
    x = torch.zeros(t, k)
    x.scatter_(1, torch.rand(t, k, generator=g).argsort(dim=1)[:, :8], torch.randint(0, 2, (t, 8), generator=g) * 2.0 - 1)
    w = torch.randint(-3, 4, (v, k), generator=g).float()
    tg = targets_for(t, v)
    want, bound = exact_bound(x.to(F64) @ w.to(F64).t(), tg)
    got = run_twice(x.to(BF), w.to(BF), tg, cuda, ranges)
    err = (got - want).abs()
    print(f"T {t} V {v} K {k} ranges {ranges}: max |err| {err.max().item():.3e}")
    assert bool((got[tg < 0] == 0).all()) and bool((err <= bound).all()), (err / bound.clamp(min=1e-300)).max().item()


@pytest.mark.parametrize("ranges", [1, 3, 0])
def test_needle(cuda, ranges):
    """Every logit 0 but one +24 in the last, ragged tile -- another range than the targets' when there are
    several, and late in the walk: a forgotten rescale or a dropped partial misses by many units."""
    t, v, k = 3, 5003, 128
    x = torch.zeros(t, k)
    x[:, 0] = 1.0
    w = torch.zeros(v, k)
    w[4999, 0] = 24.0
    tg = torch.tensor([5, 2600, 4000], dtype=torch.int32)
    want, bound = exact_bound(x.to(F64) @ w.to(F64).t(), tg)
    assert abs(want[0].item() - (-24 - math.log1p((v - 1) * math.exp(-24)))) < 1e-12
    err = (run_twice(x.to(BF), w.to(BF), tg, cuda, ranges) - want).abs()
    assert bool((err <= bound).all()), err


def test_random_bf16(cuda):
    """Random bf16 operands against the float64 log-softmax of the unrounded products.  Per row the bound is
    2 max_j (2^-9 |z_ij| + K 2^-24 sum_k |x_ik w_jk|) -- a bf16 rounding and the f32 accumulation error of a logit,
    once through the target and once through the log-sum-exp -- plus the exact cases' bound."""
    t, v, k = 300, 5003, 512
    g = torch.Generator().manual_seed(11)
    x = torch.randn(t, k, generator=g).to(BF)
    w = (torch.randn(v, k, generator=g) * 0.2).to(BF)
    tg = targets_for(t, v)
    z = x.to(F64) @ w.to(F64).t()
    want, bound = exact_bound(z, tg)
    bound = bound + 2 * (2.0 ** -9 * z.abs() + k * 2.0 ** -24 * (x.to(F64).abs() @ w.to(F64).abs().t())).max(dim=1).values
    err = (run_twice(x, w, tg, cuda, 0) - want).abs()
    print(f"random: max |err| {err.max().item():.3e}, smallest bound {bound.min().item():.3e}")
    assert bool((err <= bound).all()), (err / bound).max().item()


# ------------------------------------------------------------------ engine
NAME = "tiny-llama-d128"
ENGINE_PROMPTS = [list(range(3, 40)), [2, 4, 6], [9, 9, 2, 7, 7, 1, 30, 31, 5]]


def _engine(device, dtype, asks, **kw):
    from distributed_llms_amd.config import EngineConfig, get_model_config
    from distributed_llms_amd.engine.llm_engine import LLMEngine, ModelStage, SamplingParams
    from distributed_llms_amd.models import weights as W
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=9, dtype=torch.float32)
    ecfg = EngineConfig(model=NAME, dtype=dtype, device=device, max_batch=4, max_seq_len=256, num_kv_blocks=128,
                        graph_batch_sizes=(1, 2, 4), max_prefill_tokens=32, **kw)
    stage = ModelStage(cfg, 0, cfg.num_layers, "cuda:0" if device == "cuda" else "cpu", getattr(torch, dtype))
    eng = LLMEngine(ecfg, stage.load_hf_state(sd))
    seqs = [eng.add_request(p, SamplingParams(max_new_tokens=8, ignore_eos=True, prompt_logprobs=a))
            for p, a in zip(ENGINE_PROMPTS, asks)]
    return eng, seqs


@pytest.fixture(scope="module")
def cpu_run():
    """The float32 CPU engine's lists, and tests/test_production_shapes_gpu.py's logit error budget (0.1 x the
    std of the float32 logits), which a log-probability sees through the target and through the log-sum-exp."""
    from distributed_llms_amd.engine.batch import build_host_batch
    eng, seqs = _engine("cpu", "float32", [True, False, True], use_graphs=False)
    spread = eng.runner.execute(build_host_batch(eng.scheduler.schedule(0), eng.bm, 16)).float().std().item()
    eng, seqs = _engine("cpu", "float32", [True, False, True], use_graphs=False)
    eng.run_until_done()
    return [s.prompt_logprobs for s in seqs], 2 * 0.1 * spread, 2 * 0.013 * spread      # its max_rel, mean_rel


@pytest.mark.parametrize("lookahead", [1, 0])
@pytest.mark.parametrize("graphs", [True, False])
def test_engine_prompt_logprobs(cuda, cpu_run, graphs, lookahead):
    """Chunked prefill (37 tokens, a budget of 32) beside a request that does not ask, whose tokens stay."""
    want, bound, mean_bound = cpu_run
    kw = dict(use_graphs=graphs, kernel_knobs={"lookahead": lookahead})
    eng, seqs = _engine("cuda", "bfloat16", [True, False, True], **kw)
    plain_eng, plain = _engine("cuda", "bfloat16", [False] * 3, **kw)
    eng.run_until_done()
    plain_eng.run_until_done()
    assert bool(eng.num_lookahead) == bool(lookahead)
    assert seqs[1].output == plain[1].output and seqs[1].prompt_logprobs is None
    for s, w in zip((seqs[0], seqs[2]), (want[0], want[2])):
        assert len(s.prompt_logprobs) == len(s.prompt) and s.prompt_logprobs[0] is None
        err = max(abs(a - b) for a, b in zip(s.prompt_logprobs[1:], w[1:]))
        mean = sum(abs(a - b) for a, b in zip(s.prompt_logprobs[1:], w[1:])) / (len(w) - 1)
        print(f"max |err| {err:.3e} (bound {bound:.3e}), mean |err| {mean:.3e} (bound {mean_bound:.3e})")
        assert err <= bound and mean <= mean_bound
