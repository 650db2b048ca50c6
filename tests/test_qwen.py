"""Qwen2 / Qwen2.5 (qkv bias) and Qwen3 (per-head q / k RMSNorm) on the CPU: config round trips and
refusals, golden tokens and logits against ``transformers`` by the method of tests/test_model_vs_hf.py,
checkpoint loading and sharding, a two-stage pipeline, LoRA, and the untouched Llama path."""
import dataclasses
import json

import pytest
import torch
import transformers

from distributed_llms_amd import ops
from distributed_llms_amd.checkpoint.loader import load_model
from distributed_llms_amd.checkpoint.shard_manager import (ModelShardManager, load_shard_file,
                                                           write_synthetic_checkpoint)
from distributed_llms_amd.config import PRESETS, EngineConfig, ModelConfig, get_model_config
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.parallel.pipeline import run_loopback_pipeline

NAMES = ["tiny-qwen2", "tiny-qwen3", "tiny-qwen3-d128"]
GOLD = NAMES + ["tiny-qwen2-g7"]         # 7 q heads per kv head, as Qwen2.5-7B
PROMPTS = [[5, 17, 33, 9, 100], [7, 8, 9, 10, 11, 12, 13, 40], [3]]


# ------------------------------------------------------------------ config
def test_presets():
    q2, q3 = PRESETS["qwen2.5-7b"], PRESETS["qwen3-8b"]
    assert (q2.vocab_size, q2.hidden_size, q2.intermediate_size, q2.num_layers, q2.num_heads, q2.num_kv_heads,
            q2.head_dim, q2.max_position, q2.rope_theta, q2.norm_eps, q2.bos_token_id, q2.eos_token_id) == \
        (152064, 3584, 18944, 28, 28, 4, 128, 32768, 1e6, 1e-6, 151643, 151645)
    assert q2.attn_bias and not q2.qk_norm and q2.arch == "llama" and q2.rope_scaling is None
    assert (q3.vocab_size, q3.hidden_size, q3.intermediate_size, q3.num_layers, q3.num_heads, q3.num_kv_heads,
            q3.head_dim, q3.max_position, q3.rope_theta, q3.norm_eps, q3.bos_token_id, q3.eos_token_id) == \
        (151936, 4096, 12288, 36, 32, 8, 128, 40960, 1e6, 1e-6, 151643, 151645)
    assert q3.qk_norm and not q3.attn_bias and q3.arch == "llama"
    # public parameter counts: Qwen2.5-7B 7.62 B, Qwen3-8B 8.19 B
    assert abs(q2.param_count() / 1e9 - 7.62) < 0.01 and abs(q3.param_count() / 1e9 - 8.19) < 0.01
    t3 = PRESETS["tiny-qwen3"]
    assert t3.q_size == 512 and t3.hidden_size == 256 and t3.qk_norm and not t3.attn_bias
    t2, tl = PRESETS["tiny-qwen2"], PRESETS["tiny-llama"]
    assert dataclasses.replace(t2, name=tl.name, attn_bias=False, rope_scaling=tl.rope_scaling) == tl
    td, tld = PRESETS["tiny-qwen3-d128"], PRESETS["tiny-llama-d128"]
    assert dataclasses.replace(td, name=tld.name, attn_bias=False, qk_norm=False) == tld
    llama = PRESETS["llama3-8b"]
    assert not llama.attn_bias and not llama.qk_norm


@pytest.mark.parametrize("name", NAMES + ["qwen2.5-7b", "qwen3-8b"])
def test_hf_config_round_trip(name):
    cfg = get_model_config(name)
    hf = json.loads(json.dumps(cfg.to_hf_config()))             # what the shard manager writes and reads
    if cfg.qk_norm:
        assert hf["model_type"] == "qwen3" and hf["architectures"] == ["Qwen3ForCausalLM"]
        assert hf["attention_bias"] is cfg.attn_bias
    else:
        assert hf["model_type"] == "qwen2" and hf["architectures"] == ["Qwen2ForCausalLM"]
    assert ModelConfig.from_hf_config(hf) == cfg


def test_from_hf_config_flags():
    base = PRESETS["tiny-qwen2"].to_hf_config()
    assert ModelConfig.from_hf_config(base).attn_bias and not ModelConfig.from_hf_config(base).qk_norm
    q3 = dict(base, model_type="qwen3")
    c = ModelConfig.from_hf_config(q3)
    assert c.qk_norm and not c.attn_bias
    assert ModelConfig.from_hf_config(dict(q3, attention_bias=True)).attn_bias
    ok = dict(base, use_sliding_window=False, layer_types=["full_attention"] * 4)
    assert ModelConfig.from_hf_config(ok).attn_bias
    assert not ModelConfig.from_hf_config(dict(base, model_type="llama")).attn_bias


@pytest.mark.parametrize("extra,msg", [
    ({"use_sliding_window": True}, "sliding"),
    ({"layer_types": ["full_attention", "sliding_attention"]}, "layer_types"),
    ({"model_type": "qwen2_moe"}, "MoE"),
    ({"model_type": "qwen3_moe"}, "MoE"),
])
def test_from_hf_config_refusals(extra, msg):
    with pytest.raises(ValueError, match=msg):
        ModelConfig.from_hf_config(dict(PRESETS["tiny-qwen3"].to_hf_config(), **extra))


def test_unsupported_type_message_lists_qwen():
    with pytest.raises(ValueError, match="qwen2, qwen3"):
        ModelConfig.from_hf_config({"model_type": "phi3"})


@pytest.mark.parametrize("name", NAMES)
def test_engine_refusals(name):
    from distributed_llms_amd.parallel.tensor_parallel import TPGroup
    cfg = get_model_config(name)
    with pytest.raises(ValueError, match="fp8.*(bias|norm)"):
        LLMEngine(EngineConfig(model=name, dtype="float32", device="cpu", quant="fp8"))
    with pytest.raises(ValueError, match="fp8.*(bias|norm)"):
        ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).init_synthetic(0).quantize("fp8")
    with pytest.raises(ValueError, match="tensor parallelism.*bias shard"):
        EngineConfig(model=name).check_tensor_parallel(2)
    EngineConfig(model=name).check_tensor_parallel(1)
    with pytest.raises(ValueError, match="tensor parallelism.*bias shard"):
        ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32, tp=TPGroup(0, 2))
    EngineConfig(model="tiny-llama").check_tensor_parallel(2)       # Llama keeps both
    EngineConfig(model="tiny-llama", quant="fp8").validate()


# ------------------------------------------------------------------ weights
def test_block_shapes_names_and_param_count():
    for name in NAMES:
        cfg = get_model_config(name)
        shapes = W.block_shapes(cfg)
        assert ("bqkv" in shapes) == cfg.attn_bias and ("q_norm" in shapes) == cfg.qk_norm == ("k_norm" in shapes)
        if cfg.attn_bias:
            assert shapes["bqkv"] == (cfg.qkv_size,)
        if cfg.qk_norm:
            assert shapes["q_norm"] == shapes["k_norm"] == (cfg.head_dim,)
        blk = W.synth_block(cfg, 1, 3, torch.float32, "cpu")
        hf = W.block_to_hf(cfg, 1, blk)
        assert sorted(hf) == sorted(W.hf_block_names(cfg, 1))
        back = W.hf_to_block(cfg, 1, hf)
        assert sorted(back) == sorted(blk) and all(torch.equal(back[k], blk[k]) for k in blk)
        assert cfg.layer_param_count() == sum(t.numel() for t in blk.values())
        if cfg.attn_bias:       # concatenated in the order of wqkv
            p = "model.layers.1.self_attn."
            assert torch.equal(blk["bqkv"], torch.cat([hf[p + f"{n}_proj.bias"] for n in "qkv"]))
            assert hf[p + "k_proj.bias"].shape == (cfg.kv_size,) and blk["bqkv"].abs().max() > 0
        if cfg.qk_norm:         # 1 + N(0, 0.1), not ones, and two different vectors
            qn, kn = blk["q_norm"], blk["k_norm"]
            assert not torch.equal(qn, kn) and 0.02 < (qn - 1).std() < 0.3 and abs(qn.mean() - 1) < 0.1
            assert torch.equal(qn, W.synth_block(cfg, 1, 3, torch.float32, "cpu")["q_norm"])
    # the existing names and values do not change
    tl, t2 = get_model_config("tiny-llama"), get_model_config("tiny-qwen2")
    a, b = W.synth_block(tl, 2, 7, torch.float32, "cpu"), W.synth_block(t2, 2, 7, torch.float32, "cpu")
    assert sorted(a) == ["attn_norm", "mlp_norm", "w_down", "w_gate_up", "wo", "wqkv"]
    assert all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ golden against transformers
def _state(cfg, seed):
    """The synthetic state dict, with a non-trivial o-projection bias where the model has one."""
    sd = W.synth_hf_state_dict(cfg, seed=seed, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith("o_proj.bias"):
            sd[k] = 0.02 * torch.randn(sd[k].shape, generator=g)
    return sd


def _hf_model(cfg, sd):
    hfc = {k: v for k, v in cfg.to_hf_config().items()
           if not k.startswith("_") and k not in ("architectures", "model_type")}
    if cfg.qk_norm:
        m = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**hfc))
    else:
        m = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(**hfc))
    missing, unexpected = m.load_state_dict(sd, strict=False)       # overwrites the norm weights and biases
    assert missing == [] and unexpected == []
    return m.eval()


def _engine(name, sd, **kw):
    cfg = get_model_config(name)
    args = dict(model=name, dtype="float32", device="cpu", max_batch=8, max_seq_len=256, use_graphs=False, seed=3)
    args.update(kw)
    return LLMEngine(EngineConfig(**args), ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd))


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in GOLD:
        cfg = get_model_config(name)
        sd = _state(cfg, 3)
        out[name] = (cfg, sd, _hf_model(cfg, sd))
    return out


@pytest.mark.parametrize("name", GOLD)
def test_greedy_matches_transformers(golden, name):
    cfg, sd, m = golden[name]
    outs = _engine(name, sd).generate(PROMPTS, SamplingParams(max_new_tokens=10, ignore_eos=True))
    for p, o in zip(PROMPTS, outs):
        with torch.no_grad():
            g = m.generate(torch.tensor([p]), max_new_tokens=10, min_new_tokens=10, do_sample=False, pad_token_id=0)
        assert g[0, len(p):].tolist() == o


def _last_logits(eng, prompt):
    eng.add_request(prompt, SamplingParams(max_new_tokens=1))
    st = eng.scheduler.schedule(0)
    return eng.runner.execute(build_host_batch(st, eng.bm, 32))[0]


@pytest.mark.parametrize("name", GOLD)
def test_prefill_logits_match_transformers(golden, name):
    cfg, sd, m = golden[name]
    prompt = [1, 50, 60, 70, 80, 90]
    with torch.no_grad():
        ref = m(torch.tensor([prompt])).logits[0, -1]
    torch.testing.assert_close(_last_logits(_engine(name, sd), prompt), ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("name,drop", [("tiny-qwen2", "bqkv"), ("tiny-qwen3", "q_norm"), ("tiny-qwen3", "k_norm")])
def test_skipping_a_tensor_changes_the_tokens(golden, name, drop):
    """The synthetic bias and norm weights are not neutral: a forward without one of them decodes other tokens."""
    cfg, sd, _ = golden[name]
    p = SamplingParams(max_new_tokens=10, ignore_eos=True)
    exp = _engine(name, sd).generate(PROMPTS, p)
    eng = _engine(name, sd)
    for lw in eng.stage.layers:
        lw[drop] = torch.zeros_like(lw[drop]) if drop == "bqkv" else torch.ones_like(lw[drop])
    assert eng.generate(PROMPTS, p) != exp


# ------------------------------------------------------------------ padded GQA groups
def test_padded_heads_keep_the_outputs():
    """A GPU stage pads a GQA group the prefill attention kernels do not tile (7, as Qwen2.5-7B) to the next
    one they do with all-zero q heads; forced on a CPU stage, logits and tokens stay what they were."""
    from distributed_llms_amd.models.stage import padded_group
    assert [padded_group(g) for g in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16)] == [1, 2, 4, 4, 8, 8, 8, 8, 16, 16]
    with pytest.raises(ValueError, match="at most 16"):
        padded_group(17)
    name = "tiny-qwen2-g7"
    cfg = get_model_config(name)
    sd = _state(cfg, 3)
    plain = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)
    padded = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32, pad_heads=True).load_hf_state(sd)
    assert (plain.hq, plain.group, padded.hq, padded.group, padded.group_real) == (7, 7, 8, 8, 7)
    d, h = cfg.head_dim, cfg.hidden_size
    for a, b in zip(plain.layers, padded.layers):
        assert b["wqkv"].shape == ((8 + 2) * d, h) and b["bqkv"].shape == ((8 + 2) * d,) and b["wo"].shape == (h, 8 * d)
        assert torch.equal(b["wqkv"][:7 * d], a["wqkv"][:7 * d]) and torch.equal(b["wqkv"][8 * d:], a["wqkv"][7 * d:])
        assert not b["wqkv"][7 * d:8 * d].any() and not b["bqkv"][7 * d:8 * d].any() and not b["wo"][:, 7 * d:].any()
        assert torch.equal(b["wo"][:, :7 * d], a["wo"]) and torch.equal(b["bqkv"][8 * d:], a["bqkv"][7 * d:])
    synth = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32, pad_heads=True).init_synthetic(3)
    assert synth.layers[0]["wqkv"].shape == ((8 + 2) * d, h)
    kw = dict(model=name, dtype="float32", device="cpu", max_batch=8, max_seq_len=256, use_graphs=False)
    e0, e1 = LLMEngine(EngineConfig(**kw), plain), LLMEngine(EngineConfig(**kw), padded)
    prompt = [1, 50, 60, 70, 80, 90]
    torch.testing.assert_close(_last_logits(e1, prompt), _last_logits(e0, prompt), atol=1e-5, rtol=1e-5)
    p = SamplingParams(max_new_tokens=10, ignore_eos=True)
    e0, e1 = LLMEngine(EngineConfig(**kw), plain), LLMEngine(EngineConfig(**kw), padded)
    assert e1.generate(PROMPTS, p) == e0.generate(PROMPTS, p)
    # a supported group is left alone; what a padded stage refuses
    same = ModelStage(get_model_config("tiny-qwen2"), 0, 4, "cpu", torch.float32, pad_heads=True)
    assert same.hq == 4 and same.group == same.group_real == 2
    with pytest.raises(ValueError, match="LoRA.*pads its GQA group"):
        padded.load_lora(EngineConfig(lora_modules={"a": "synthetic:8:1"}, **kw))
    with pytest.raises(ValueError, match="sub-layer cuts.*padded GQA group"):
        ModelStage(cfg, 0, 2, "cpu", torch.float32, units=(0, 6), unit_group=5, pad_heads=True)


# ------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("safetensors", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_directory_loads_and_shards(tmp_path, name, safetensors):
    cfg = get_model_config(name)
    path = write_synthetic_checkpoint(name, str(tmp_path / name), seed=3, safetensors=safetensors)
    with open(tmp_path / name / "config.json") as f:
        assert json.load(f)["model_type"] == ("qwen3" if cfg.qk_norm else "qwen2")
    sd = W.synth_hf_state_dict(cfg, seed=3, dtype=torch.float32)
    stage, _ = load_model(path, device_map="cpu", dtype="float32")
    assert stage.cfg == dataclasses.replace(cfg, name=stage.cfg.name)
    want = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)
    for a, b in zip(stage.layers, want.layers):
        assert sorted(a) == sorted(b) == sorted(W.block_shapes(cfg)) and all(torch.equal(a[k], b[k]) for k in a)
    mgr = ModelShardManager(path, 2)
    shard_dir = mgr.shard_model(write_safetensors=safetensors)
    assert get_model_config(shard_dir) == stage.cfg                 # shards/config.json round trip
    shards = [load_shard_file(p) for p in mgr.get_shard_paths()]
    assert sorted(k for s in shards for k in s) == sorted(sd)
    for l in range(cfg.num_layers):                                  # every block key in its layer's shard
        home = shards[mgr.plan.stage_of_layer(l)]
        assert all(k in home and torch.equal(home[k], sd[k]) for k in W.hf_block_names(cfg, l))
    full, hf = ModelShardManager.reconstruct_model(mgr.get_shard_paths(), shard_dir + "/config.json")
    p = SamplingParams(max_new_tokens=6, ignore_eos=True)
    a = LLMEngine(EngineConfig(model=name, shard_dir=shard_dir, dtype="float32", device="cpu", use_graphs=False,
                               max_seq_len=256),
                  ModelStage(stage.cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(full)).generate(PROMPTS, p)
    assert a == _engine(name, sd).generate(PROMPTS, p)


def test_indexed_safetensors_checkpoint_loads(tmp_path):
    from safetensors.torch import save_file
    name = "tiny-qwen3-d128"
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=4, dtype=torch.float32)
    keys = sorted(sd)
    files = {"model-00001-of-00002.safetensors": keys[::2], "model-00002-of-00002.safetensors": keys[1::2]}
    for f, ks in files.items():
        save_file({k: sd[k].contiguous() for k in ks}, str(tmp_path / f))
    with open(tmp_path / "model.safetensors.index.json", "w") as f:
        json.dump({"weight_map": {k: fn for fn, ks in files.items() for k in ks}}, f)
    with open(tmp_path / "config.json", "w") as f:
        json.dump(cfg.to_hf_config(), f)
    stage, _ = load_model(str(tmp_path), device_map="cpu", dtype="float32")
    want = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)
    for a, b in zip(stage.layers, want.layers):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    ModelShardManager(str(tmp_path), 2).shard_model()


# ------------------------------------------------------------------ pipeline, LoRA, the Llama path
def _pp_ecfg(name):
    return EngineConfig(model=name, dtype="float32", device="cpu", max_batch=4, max_seq_len=128, use_graphs=False,
                        num_kv_blocks=128, seed=3)


@pytest.mark.parametrize("units", ["", "5:0,11;11,20"], ids=["planned", "cut-after-qkv"])
@pytest.mark.parametrize("name", NAMES)
def test_two_stage_pipeline_matches_one_stage(monkeypatch, name, units):
    """``cut-after-qkv``: stage 1 starts at atom 1 of layer 2, so it receives qkv with the bias and the norms
    already applied."""
    prompts = [[i + 1, 2 * i + 3, 5, 7, 11 + i] for i in range(6)]
    p = SamplingParams(max_new_tokens=8, ignore_eos=True)
    exp = LLMEngine(_pp_ecfg(name)).generate(prompts, p)
    if units:
        monkeypatch.setenv("DLLM_PP_UNITS", units)
    outs, drv, plan = run_loopback_pipeline(_pp_ecfg(name), 2, prompts, p, device="cpu")
    assert outs == exp and drv.num_steps > 0
    if units:
        assert plan.group == 5 and plan.units == ((0, 11), (11, 20))


def test_adapter_engine_matches_merged_weights():
    import test_lora as tl
    name, spec = "tiny-qwen2", "synthetic:8:11"
    cfg = get_model_config(name)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    kw = dict(num_kv_blocks=128, seed=0)
    eng = _engine(name, sd, lora_modules={"alpha": spec}, **kw)
    merged = _engine(name, tl._merged_state(cfg, sd, spec), **kw)
    base = _engine(name, sd, **kw)
    la = tl._prefill_logits(eng, tl.PROMPTS, ["alpha"] * 3)
    lm = tl._prefill_logits(merged, tl.PROMPTS, [None] * 3)
    lb = tl._prefill_logits(base, tl.PROMPTS, [None] * 3)
    torch.testing.assert_close(la, lm, atol=1e-4, rtol=1e-4)
    assert (la - lb).abs().max().item() > 1e-2, "the adapter must change the logits"
    ta = eng.generate(tl.PROMPTS, tl._params("alpha"))
    assert ta == merged.generate(tl.PROMPTS, tl._params(None)) and all(len(t) == 8 for t in ta)
    assert ta != base.generate(tl.PROMPTS, tl._params(None))


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-mixtral"])
def test_llama_path_calls_nothing_new(monkeypatch, name):
    p = SamplingParams(max_new_tokens=6, ignore_eos=True)
    ecfg = EngineConfig(model=name, dtype="float32", device="cpu", max_batch=4, max_seq_len=128, use_graphs=False)
    exp = LLMEngine(ecfg).generate(PROMPTS, p)

    def boom(*a, **k):
        raise AssertionError("qkv_prep_ called on a model with neither flag")
    monkeypatch.setattr(ops, "qkv_prep_", boom)
    assert LLMEngine(ecfg).generate(PROMPTS, p) == exp
    assert sorted(W.block_shapes(get_model_config(name))) == sorted(
        k for k in W.block_shapes(get_model_config(name)) if k not in ("bqkv", "q_norm", "k_norm", "bo"))
    with pytest.raises(AssertionError, match="neither flag"):        # the hook is live: a Qwen engine does call it
        LLMEngine(dataclasses.replace(ecfg, model="tiny-qwen2")).generate(PROMPTS, p)


# ------------------------------------------------------------------ padded groups with several kv heads
@pytest.mark.parametrize("bias", [False, True])
def test_padded_heads_interleave_per_kv_group(monkeypatch, bias):
    """6 q heads over 2 kv heads (group 3 -> 4): the zero heads sit at head indices 3 and 7, one behind each kv
    group, not at the end of the q block.  Qwen3 norms, with and without the attention biases."""
    from distributed_llms_amd import config
    name = "tiny-qwen3-g3"
    cfg = dataclasses.replace(PRESETS["tiny-qwen3"], name=name, num_heads=6, num_kv_heads=2, attn_bias=bias)
    monkeypatch.setitem(config.PRESETS, name, cfg)
    sd = _state(cfg, 4)
    plain = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)
    padded = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32, pad_heads=True).load_hf_state(sd)
    assert (plain.hq, padded.hq, padded.hkv, padded.group, padded.group_real) == (6, 8, 2, 4, 3)
    d, h = cfg.head_dim, cfg.hidden_size
    real, zero = [0, 1, 2, 4, 5, 6], [3, 7]
    for a, b in zip(plain.layers, padded.layers):
        wq = b["wqkv"][:8 * d].view(8, d, h)
        assert torch.equal(wq[real], a["wqkv"][:6 * d].view(6, d, h)) and not wq[zero].any()
        assert torch.equal(b["wqkv"][8 * d:], a["wqkv"][6 * d:])
        wo = b["wo"].view(h, 8, d)
        assert torch.equal(wo[:, real], a["wo"].view(h, 6, d)) and not wo[:, zero].any()
        if bias:
            bq = b["bqkv"][:8 * d].view(8, d)
            assert torch.equal(bq[real], a["bqkv"][:6 * d].view(6, d)) and not bq[zero].any()
            assert torch.equal(b["bqkv"][8 * d:], a["bqkv"][6 * d:]) and torch.equal(b["bo"], a["bo"])
    kw = dict(model=name, dtype="float32", device="cpu", max_batch=8, max_seq_len=256, use_graphs=False)
    prompt = [1, 50, 60, 70, 80, 90]
    torch.testing.assert_close(_last_logits(LLMEngine(EngineConfig(**kw), padded), prompt),
                               _last_logits(LLMEngine(EngineConfig(**kw), plain), prompt), atol=1e-5, rtol=1e-5)
    p = SamplingParams(max_new_tokens=10, ignore_eos=True)
    plain = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd)
    padded = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32, pad_heads=True).load_hf_state(sd)
    exp = LLMEngine(EngineConfig(**kw), plain).generate(PROMPTS, p)
    assert LLMEngine(EngineConfig(**kw), padded).generate(PROMPTS, p) == exp
    m = _hf_model(cfg, sd)                              # and both are what transformers computes
    for q, o in zip(PROMPTS, exp):
        with torch.no_grad():
            g = m.generate(torch.tensor([q]), max_new_tokens=10, min_new_tokens=10, do_sample=False, pad_token_id=0)
        assert g[0, len(q):].tolist() == o


# ------------------------------------------------------------------ sampled requests and the vocabulary
def test_sampled_requests_on_an_oversize_vocabulary_are_refused_at_admission(monkeypatch):
    """Both full-size vocabularies exceed the fused sampler's row.  A request with temperature > 0 is refused
    when it is admitted, with the reason, wherever the fused sampler would draw it; greedy requests and
    stages that sample on the host are admitted."""
    from distributed_llms_amd import knobs
    from distributed_llms_amd.engine import llm_engine, sequence as S
    from distributed_llms_amd.master.node import MasterNode, WorkerFailure
    assert S.SAMPLE_MAX_VOCAB == ops.SAMPLE_MAX_VOCAB
    for name in ("qwen2.5-7b", "qwen3-8b"):
        v = PRESETS[name].vocab_size
        assert v > S.SAMPLE_MAX_VOCAB
        for params in (SamplingParams(temperature=0.7), {"temperature": 0.7}):
            with pytest.raises(ValueError, match=f"vocabulary of {v} exceeds.*fused GPU sampler"):
                S.validate_sampling(params, v, True)
            S.validate_sampling(params, v, False)                       # host sampler
            S.validate_sampling(params, PRESETS["llama3-8b"].vocab_size, True)
        S.validate_sampling(SamplingParams(temperature=0.0), v, True)   # greedy
        S.validate_sampling({}, v, True)
    assert S.fused_sampler_serves("cuda:0", torch.bfloat16) and S.fused_sampler_serves("cuda", "bfloat16")
    assert not S.fused_sampler_serves("cpu", torch.bfloat16) and not S.fused_sampler_serves("cuda", "float32")
    assert not S.fused_sampler_serves("cuda", "bfloat16", {"fused_sampler": False})
    with knobs.override(fused_sampler=False):
        assert not S.fused_sampler_serves("cuda", "bfloat16")
    # the engine: admission, not a running step, refuses; the engine goes on serving
    cfg = get_model_config("tiny-qwen2")
    eng = _engine("tiny-qwen2", W.synth_hf_state_dict(cfg, seed=3, dtype=torch.float32))
    p = SamplingParams(max_new_tokens=4, ignore_eos=True)
    exp = eng.generate(PROMPTS, p)
    eng.add_request(PROMPTS[0], SamplingParams(max_new_tokens=2, temperature=0.7))      # CPU stage: host sampler
    eng.run_until_done()
    monkeypatch.setattr(S, "SAMPLE_MAX_VOCAB", 100)
    monkeypatch.setattr(llm_engine, "fused_sampler_serves", lambda *a, **k: True)
    with pytest.raises(ValueError, match="vocabulary of 512 exceeds"):
        eng.add_request(PROMPTS[0], SamplingParams(max_new_tokens=2, temperature=0.7))
    assert not eng.has_work() and eng.generate(PROMPTS, p) == exp
    monkeypatch.undo()
    # the master refuses before it dispatches, by its configured device
    gpu = MasterNode("127.0.0.1", 0, EngineConfig(model="synthetic:qwen3-8b", device="cuda", dtype="bfloat16"))
    gpu.model_config = get_model_config("qwen3-8b")
    with pytest.raises(ValueError, match="vocabulary of 151936 exceeds"):
        gpu.submit([1, 2, 3], {"temperature": 0.8, "max_new_tokens": 4})
    with pytest.raises(WorkerFailure):                     # greedy passes validation (no pipeline here)
        gpu.submit([1, 2, 3], {"max_new_tokens": 4})
    cpu = MasterNode("127.0.0.1", 0, EngineConfig(model="synthetic:qwen3-8b", device="cpu", dtype="float32"))
    cpu.model_config = get_model_config("qwen3-8b")
    with pytest.raises(WorkerFailure):
        cpu.submit([1, 2, 3], {"temperature": 0.8, "max_new_tokens": 4})


def test_worker_answers_a_refused_request_and_keeps_serving(monkeypatch):
    """Stage 0's serve loop: a request its engine refuses at admission gets an ERROR reply with the reason;
    the request queued behind it is served."""
    import threading
    import time
    from distributed_llms_amd.engine import llm_engine, sequence as S
    from distributed_llms_amd.worker.node import WorkerNode
    cfg = get_model_config("tiny-qwen2")
    eng = _engine("tiny-qwen2", W.synth_hf_state_dict(cfg, seed=3, dtype=torch.float32))
    exp = eng.generate(PROMPTS[:1], SamplingParams(max_new_tokens=4, ignore_eos=True))[0]
    monkeypatch.setattr(S, "SAMPLE_MAX_VOCAB", 100)
    monkeypatch.setattr(llm_engine, "fused_sampler_serves", lambda *a, **k: True)
    sent = []

    class Proto:
        def send_message(self, sock, command, payload=b"", metadata=None):
            sent.append((sock, command, dict(metadata or {})))

    w = WorkerNode.__new__(WorkerNode)
    w.running, w.driver, w.engine, w.proto = True, None, eng, Proto()
    w._req_cv = threading.Condition()
    w._pending = [("a", "t1", PROMPTS[0], SamplingParams(max_new_tokens=4, temperature=0.7), False),
                  ("b", "t2", PROMPTS[0], SamplingParams(max_new_tokens=4, ignore_eos=True), False)]
    th = threading.Thread(target=w._serve_loop, daemon=True)
    th.start()
    t0 = time.time()
    while not any(c == "RESULT" for _, c, _ in sent) and th.is_alive() and time.time() - t0 < 60:
        time.sleep(0.01)
    w.running = False
    with w._req_cv:
        w._req_cv.notify_all()
    th.join(10)
    assert not th.is_alive()
    assert [(s, c) for s, c, _ in sent] == [("a", "ERROR"), ("b", "RESULT")]
    assert sent[0][2]["task_id"] == "t1" and "vocabulary of 512 exceeds" in sent[0][2]["error"]
    assert sent[1][2]["task_id"] == "t2" and sent[1][2]["num_tokens"] == len(exp)
