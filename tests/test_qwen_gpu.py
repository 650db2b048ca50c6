"""csrc/kernels/qkv_prep.hip on the cases of tests/qwen_cases.py (bit for bit where the f32 sum is exact,
within half a bf16 ulp + 2^-12 of fp64 for the normed heads, sentinels in the untouched v slots, guard rows
around the tensor, equal bits from a second launch), and the Qwen2 / Qwen3 engines on the GPU: bf16 against
the CPU float32 engine, graphs against eager, lookahead on against off, two stages against one (gfx950 only).

What launches what
  qkv_prep_kernel<8>  / <16>   test_qkv_prep at head_dim 64 / 128: one block and several, a last wave that is
                               partly idle (T = 1, 3), all slots (bias) or the q and k slots only (norm)
  the second vector per lane and the grid-stride loop's second trip: test_qkv_prep_past_the_grid_cap"""
import pytest
import torch

import qwen_cases as qc
from distributed_llms_amd import ops
from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage

pytestmark = pytest.mark.gpu

# tiny-qwen2-g7: 7 q heads per kv head (Qwen2.5-7B's group), which the GPU stage pads to 8 with zero heads
NAMES = ["tiny-qwen2", "tiny-qwen3", "tiny-qwen3-d128", "tiny-qwen2-g7"]
I16 = torch.int16


def _check(case):
    buf, y = qc.run(case, ops.qkv_prep_, device="cuda")
    msg = qc.mismatch(case, y)
    assert msg is None, msg
    qc.assert_guards(buf.cpu())
    buf2, _ = qc.run(case, ops.qkv_prep_, device="cuda")
    assert torch.equal(buf, buf2), "a second launch gave other bits"


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("tokens", qc.TOKENS)
@pytest.mark.parametrize("shape", qc.SHAPES, ids=str)
def test_qkv_prep(cuda, shape, tokens, kind):
    _check(qc.prep_case(*shape, tokens, kind))


@pytest.mark.parametrize("shape,tokens,kind", [((32, 8, 128), 1400, "both"), ((8, 2, 64), 13200, "norm")], ids=str)
def test_qkv_prep_past_the_grid_cap(cuda, shape, tokens, kind):
    """More than 2 x 2048 x 256 vectors: every lane's second vector and a second trip of the grid-stride loop."""
    hq, hkv, d = shape
    slots = hq + 2 * hkv if kind == "both" else hq + hkv
    assert tokens * slots * d // 8 > 2 * 2048 * 256
    _check(qc.prep_case(*shape, tokens, kind))


def test_qkv_prep_single_norms_leave_the_other_heads(cuda):
    """Only q_w: the k and v slots keep their bits; only k_w: the q and v slots do."""
    hq, hkv, d, t = 4, 2, 64, 17
    case = qc.prep_case(hq, hkv, d, t, "norm")
    x = case.qkv.cuda()
    for q_w, k_w, lo, hi in ((case.q_w.cuda(), None, 0, hq), (None, case.k_w.cuda(), hq, hq + hkv)):
        y = ops.qkv_prep_(x.clone(), None, q_w, k_w, hq, hkv, d, qc.EPS).cpu().view(t, -1, d)
        keep = torch.ones(hq + 2 * hkv, dtype=torch.bool)
        keep[lo:hi] = False
        assert torch.equal(y[:, keep].view(I16), case.qkv.view(t, -1, d)[:, keep].view(I16))
        msg = qc.rel_mismatch(y[:, lo:hi], case.ref64[:, lo:hi], kinds=case.rows)
        assert msg is None, msg
    y = ops.qkv_prep_(x.clone(), None, None, None, hq, hkv, d, qc.EPS)          # nothing to do: no launch
    assert torch.equal(y.view(I16), x.view(I16))


def test_qkv_prep_refuses_other_head_sizes(cuda):
    with pytest.raises(ValueError, match="head_dim"):
        ops.qkv_prep_(torch.zeros(2, 4 * 32, dtype=torch.bfloat16, device="cuda"),
                      torch.zeros(4 * 32, dtype=torch.bfloat16, device="cuda"), None, None, 2, 1, 32, 1e-6)
    with pytest.raises(TypeError):
        ops.qkv_prep_(torch.zeros(2, 4 * 64, device="cuda"), torch.zeros(4 * 64, device="cuda"), None, None, 2, 1, 64,
                      1e-6)


# ------------------------------------------------------------------ engines
def _engines(name, graphs=True, cpu=True):
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    e_cpu = LLMEngine(EngineConfig(model=name, dtype="float32", device="cpu", max_batch=8, max_seq_len=512,
                                   use_graphs=False),
                      ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)) if cpu else None
    e_gpu = LLMEngine(EngineConfig(model=name, dtype="bfloat16", device="cuda", max_batch=8, max_seq_len=512,
                                   use_graphs=graphs, num_kv_blocks=256, graph_batch_sizes=(1, 2, 4, 8)),
                      ModelStage(cfg, 0, cfg.num_layers, "cuda", torch.bfloat16).load_hf_state(sd))
    return e_cpu, e_gpu


@pytest.mark.parametrize("name", NAMES)
def test_prefill_logits_gpu_vs_cpu(cuda, name):
    """The rule of tests/test_engine_gpu.py for tiny-llama."""
    e_cpu, e_gpu = _engines(name, graphs=False)
    prompts = [[1, 5, 9, 200, 37, 44, 45, 46, 47, 48], [3, 4], list(range(10, 80))]
    outs = []
    for eng in (e_cpu, e_gpu):
        for p in prompts:
            eng.add_request(p, SamplingParams(max_new_tokens=1))
        st = eng.scheduler.schedule(0)
        outs.append(eng.runner.execute(build_host_batch(st, eng.bm, 32)).float().cpu())
    torch.testing.assert_close(outs[1], outs[0], atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("name", NAMES)
def test_graph_decode_matches_eager(cuda, name):
    _, e_eager = _engines(name, graphs=False, cpu=False)
    _, e_graph = _engines(name, graphs=True, cpu=False)
    prompts = [[1, 5, 9, 200], [3, 4, 7], list(range(10, 70)), [8] * 33, [9, 9, 9]]
    p = SamplingParams(max_new_tokens=24, ignore_eos=True)
    assert e_eager.generate(prompts, p) == e_graph.generate(prompts, p)
    assert e_graph.runner.graphs.graphs, "decode never went through a captured graph"


@pytest.mark.parametrize("name", NAMES)
def test_lookahead_decode_matches_synchronous(cuda, name):
    prompts = [[1, 5, 9, 200], [3, 4, 7], list(range(10, 70)), [8] * 33, [9, 9, 9], [2, 3]]
    lens = [5, 17, 24, 9, 24, 2]

    def run(lookahead):
        _, eng = _engines(name, graphs=True, cpu=False)
        eng.lookahead = lookahead
        seqs = [eng.add_request(p, SamplingParams(max_new_tokens=n, ignore_eos=True)) for p, n in zip(prompts, lens)]
        eng.run_until_done()
        return [s.output for s in seqs], eng.num_lookahead

    sync, n0 = run(False)
    la, n1 = run(True)
    assert n0 == 0 and n1 > 0, "lookahead path never taken"
    assert la == sync


@pytest.mark.parametrize("name", NAMES)
def test_two_stage_pipeline_matches_one_stage(cuda, name):
    from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=9, dtype=torch.float32)
    ecfg = EngineConfig(model=name, dtype="bfloat16", device="cuda", max_batch=4, max_seq_len=256,
                        num_kv_blocks=128, graph_batch_sizes=(1, 2, 4))
    prompts = [[i + 1, 2 * i + 3, 5, 7, 11 + i] for i in range(10)]
    p = SamplingParams(max_new_tokens=12, ignore_eos=True)
    ref = LLMEngine(ecfg, ModelStage(cfg, 0, cfg.num_layers, "cuda", torch.bfloat16).load_hf_state(sd)).generate(prompts, p)
    outs, drv, plan = run_loopback_pipeline(ecfg, 2, prompts, p, device="cuda", hf_state=sd)
    assert outs == ref
    assert drv.num_steps > 0


def test_sampled_request_on_an_oversize_vocabulary_is_refused_at_admission(cuda, monkeypatch):
    """The fused sampler holds rows of at most ops.SAMPLE_MAX_VOCAB entries (both full-size Qwen vocabularies
    exceed it).  The GPU engine refuses such a sampled request in add_request, before any step runs, and
    goes on serving; with the limit where it is, the tiny model samples through the kernel."""
    from distributed_llms_amd.engine import sequence as S
    _, eng = _engines("tiny-qwen2", graphs=True, cpu=False)
    prompts = [[1, 5, 9, 200], [3, 4, 7]]
    greedy = SamplingParams(max_new_tokens=8, ignore_eos=True)
    sampled = SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=0.8, seed=11)
    exp = eng.generate(prompts, greedy)
    drawn = eng.generate(prompts, sampled)
    assert all(len(o) == 8 for o in drawn)
    monkeypatch.setattr(S, "SAMPLE_MAX_VOCAB", 100)          # the tiny vocabulary (512) is now oversize
    with pytest.raises(ValueError, match="vocabulary of 512 exceeds.*fused GPU sampler"):
        eng.add_request(prompts[0], sampled)
    assert not eng.has_work()
    assert eng.generate(prompts, greedy) == exp
    monkeypatch.undo()
    assert eng.generate(prompts, sampled) == drawn
