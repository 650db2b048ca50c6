"""Int4 (W4A16) weights on the CPU: packing, the quantizer, the reference op (ops/reference.py "int4 weights"),
quant="int4" and its refusals, and the float32 engine against the same engine on the dequantized weights."""
import dataclasses

import pytest
import torch

from distributed_llms_amd import config, ops
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.batch import build_host_batch
from distributed_llms_amd.engine.llm_engine import LLMEngine, build_stage
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.ops import int4

MODEL = "tiny-llama-d128"      # hidden 512, intermediate 1024, qkv 768: every projection a multiple of 128


def test_every_code_round_trips_through_pack_and_dequantize():
    g = torch.Generator().manual_seed(0)
    u = torch.randint(0, 16, (256, 384), generator=g, dtype=torch.uint8)
    u[0, :16] = torch.arange(16, dtype=torch.uint8)
    s = (torch.rand(256, 3, generator=g) + 0.5).to(torch.bfloat16)
    w = int4.from_codes(u, s)
    assert w.shape == (256, 384) and w.nbytes() == 256 * 384 // 2 + 256 * 3 * 2
    assert torch.equal(int4.unpack(w.packed), u) and torch.equal(w.scales(), s)
    assert torch.equal(w.dequantize(), (u.float() - 8) * s.float().repeat_interleave(128, 1))
    # the kernel's order: lane r + 16 q of block (t, g), word j, code e of k = 32 j + 8 q + e at bit 4 (e / 2) + 16 (e % 2)
    words = w.packed.view(16, 3, 64, 4, 4).int()
    word = sum(words[1, 2, 5 + 16 * 3, 2, b].item() << (8 * b) for b in range(4))
    assert [(word >> (4 * (e // 2) + 16 * (e % 2))) & 15 for e in range(8)] == u[21, 256 + 64 + 24:][:8].tolist()


def test_quantizer_maps_absmax_to_seven_and_zero_groups_to_unit_scale():
    torch.manual_seed(1)
    w = torch.randn(128, 256)
    w[5, :128] = 0
    q = int4.quantize_weight(w)
    u, s = q.codes().int() - 8, q.scales()
    assert u.min() >= -8 and u.max() <= 7 and s[5, 0] == 1 and (u[5, :128] == 0).all()
    amax = w.view(128, 2, 128).abs().amax(2)
    assert torch.equal(s.float() == 1, amax == 0) and torch.equal(s[amax > 0], (amax / 7).to(torch.bfloat16)[amax > 0])
    at = w.view(128, 2, 128).abs().argmax(2, keepdim=True)
    assert (u.view(128, 2, 128).gather(2, at).abs().squeeze(2)[amax > 0] == 7).all()
    assert (q.dequantize() - w).abs().max() <= 0.51 * s.float().max()


def test_reference_op_on_hand_made_rows():
    u = torch.full((128, 256), 8, dtype=torch.uint8)
    u[0, 0], u[0, 130], u[3, 255] = 15, 0, 9          # +7, -8, +1
    s = torch.ones(128, 2, dtype=torch.bfloat16)
    s[0, 1], s[3, 1] = 0.5, 3.0
    x = torch.zeros(2, 256)
    x[0, 0], x[0, 130], x[1, 255] = 2.0, 1.0, -4.0
    y = ops.linear(x, int4.from_codes(u, s))
    want = torch.zeros(2, 128)
    want[0, 0], want[1, 3] = 2 * 7 - 8 * 0.5, -4 * 3.0
    assert torch.equal(y, want)
    with pytest.raises(ValueError):
        ops.linear(x, int4.from_codes(u, s), bias=torch.zeros(128))


def test_int4_validates_and_refuses_what_is_not_wired(monkeypatch):
    EngineConfig(model=MODEL, quant="int4").validate()
    for kw in (dict(model="tiny-gpt2"), dict(model="tiny-mixtral"), dict(model="tiny-qwen2"), dict(model="tiny-qwen3"),
               dict(lora_modules={"a": "synthetic:8:1"})):
        with pytest.raises(ValueError):
            EngineConfig(**{"model": MODEL, "quant": "int4", **kw}).validate()
    with pytest.raises(ValueError, match="tp > 1"):
        EngineConfig(model=MODEL, quant="int4").check_tensor_parallel(2)
    odd = dataclasses.replace(config.PRESETS[MODEL], name="odd", hidden_size=192, intermediate_size=320, head_dim=48)
    monkeypatch.setitem(config.PRESETS, "odd", odd)
    with pytest.raises(ValueError, match="converted no weight"):
        build_stage(EngineConfig(model="odd", dtype="float32", device="cpu", quant="int4"))
    monkeypatch.setenv("DLLM_PP_FINE", "1")
    with pytest.raises(ValueError, match="DLLM_PP_FINE"):
        EngineConfig(model=MODEL, quant="int4").validate()


def test_cpu_engine_equals_the_engine_on_dequantized_weights():
    base = EngineConfig(model=MODEL, dtype="float32", device="cpu", max_batch=4, max_seq_len=64, num_kv_blocks=64,
                        use_graphs=False)
    q = LLMEngine(base.apply_overrides(quant="int4"))
    layers = q.stage.layers
    assert sum(isinstance(t, int4.Int4Weight) for lw in layers for t in lw.values()) == 4 * len(layers)
    plain = build_stage(base)
    assert int4.quantize_layers([dict(lw) for lw in plain.layers]) == 4 * len(layers)
    for lw, lq in zip(plain.layers, layers):
        for k in int4.QUANT_KEYS:
            lw[k] = lq[k].dequantize()
    prompts, sp = [[1, 2, 3, 4], [5, 6, 7]], SamplingParams(max_new_tokens=6, ignore_eos=True, logprobs=0)
    p = LLMEngine(base, plain)
    assert q.generate(prompts, sp) == p.generate(prompts, sp)
    logits = []
    for eng in (q, p):
        eng.add_request(prompts[0], SamplingParams(max_new_tokens=1))
        logits.append(eng.runner.execute(build_host_batch(eng.scheduler.schedule(0), eng.bm, 32)))
    assert torch.equal(*logits)
