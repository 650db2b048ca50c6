"""AWQ / GPTQ 4-bit checkpoints on the CPU: the formats of ops/reference.py against packers written here, the
loader (models/weights.py hf_to_block_w4) through the engine, and what the configuration refuses."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import teacher_forced as tf
from distributed_llms_amd.config import EngineConfig, ModelConfig, get_model_config
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.ops import int4, reference as ref

FORMATS = ("awq", "gptq", "gptq_v2")
QCONFIG = {"awq": {"quant_method": "awq", "bits": 4, "group_size": 128, "zero_point": True, "version": "gemm"},
           "gptq": {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False, "sym": False},
           "gptq_v2": {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False,
                       "checkpoint_format": "gptq_v2"}}


def _words(v, order=range(8)):
    """uint8 [..., 8 C] -> int32 [..., C]: value order[i] of every eight at bit 4 i."""
    v = v.reshape(*v.shape[:-1], -1, 8).astype(np.uint32)[..., list(order)]
    return (v << (4 * np.arange(8, dtype=np.uint32))).sum(-1, dtype=np.uint32).view(np.int32)


def checkpoint(fmt, u, z, s):
    """Codes u [N, K], zeros z [N, G] (uint8) and scales s [N, G] as the format stores them."""
    un, zn = u.numpy(), z.numpy()
    if fmt == "awq":
        qw, qz = _words(un.T, ref.AWQ_ORDER), _words(zn.T, ref.AWQ_ORDER)
    else:
        qw, qz = _words(un).T, _words((zn.T - (fmt == "gptq")) & 15)
    return torch.from_numpy(np.ascontiguousarray(qw)), torch.from_numpy(np.ascontiguousarray(qz)), s.t().contiguous()


def random_weight(n, k, seed, pow2=False):
    """u, z, s: every code and every zero 0..15 occurs; f16 scales (``pow2``: powers of two)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (n, k // 128), generator=g, dtype=torch.uint8)
    u[:, :16] = torch.arange(16, dtype=torch.uint8)
    z[:16, 0] = torch.arange(16, dtype=torch.uint8)
    e = torch.exp2(torch.randint(-4, 3, (n, k // 128), generator=g).float())
    return u, z, (e if pow2 else e * (1 + torch.rand(n, k // 128, generator=g))).to(torch.float16)


@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_round_trip_and_stack_along_n(fmt):
    a, b = random_weight(128, 256, 1), random_weight(256, 256, 2)
    for want in (a, b):
        assert all(torch.equal(x, y) for x, y in zip(ref.unpack_w4(fmt, *checkpoint(fmt, *want)), want))
    w = int4.from_checkpoint([checkpoint(fmt, *a), checkpoint(fmt, *b)], fmt)
    u, z, s = (torch.cat(p) for p in zip(a, b))
    assert w.shape == (384, 256) and w.scales().dtype == torch.float16
    assert torch.equal(w.codes(), u) and torch.equal(w.zeros(), z) and torch.equal(w.scales(), s)
    assert torch.equal(w.dequantize(), (u.float() - z.float().repeat_interleave(128, 1)) * s.float().repeat_interleave(128, 1))


def write_quantized(path, fmt, seed=5):
    """A tiny-llama@2l checkpoint directory whose projections are quantized round-to-nearest with zero points, in
    format ``fmt``; -> (cfg, the HF state dict of the dequantized weights)."""
    cfg = get_model_config("tiny-llama@2l")
    sd, q = W.synth_hf_state_dict(cfg, seed=seed, dtype=torch.float32), {}
    for key, w in list(sd.items()):
        if not key.endswith("_proj.weight"):
            q[key] = w
            continue
        n, k = w.shape
        wg = w.view(n, k // 128, 128)
        lo, hi = wg.amin(2).clamp(max=0), wg.amax(2).clamp(min=0)
        s = ((hi - lo) / 15).to(torch.float16)
        z = torch.round(-lo / s.float()).clamp(0, 15)
        u = (torch.round(wg / s.float()[..., None]) + z[..., None]).clamp(0, 15).view(n, k).to(torch.uint8)
        sd[key] = ref.dequantize_w4(u, s, z.to(torch.uint8))
        base = key[:-len("weight")]
        q[base + "qweight"], q[base + "qzeros"], q[base + "scales"] = checkpoint(fmt, u, z.to(torch.uint8), s)
        if fmt != "awq":       # what GPTQ writers add
            q[base + "g_idx"], q[base + "bias"] = (torch.arange(k) // 128).int(), torch.zeros(n, dtype=torch.float16)
    path.mkdir(parents=True, exist_ok=True)
    save_file(q, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps(dict(cfg.to_hf_config(), quantization_config=QCONFIG[fmt])))
    return cfg, sd


def prefill_logits(eng, prompts):
    rec = tf.record(eng)
    eng.generate(prompts, tf.greedy(1))
    return torch.stack([r.logits for r in sorted(rec.finish(), key=lambda r: len(r.seq.prompt))])


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_loads_the_checkpoint_directory(tmp_path, fmt):
    cfg, sd = write_quantized(tmp_path / fmt, fmt)
    kw = dict(device="cpu", dtype="float32", max_batch=4, max_seq_len=64, num_kv_blocks=16)
    eng = LLMEngine(EngineConfig(model=str(tmp_path / fmt), quant="int4", **kw))
    assert eng.mcfg.quantization == QCONFIG[fmt] and get_model_config(str(tmp_path / fmt)) == eng.mcfg
    assert all(isinstance(lw[k], int4.Int4Weight) and lw[k].zeros() is not None
               for lw in eng.stage.layers for k in W.W4_PROJECTIONS)
    want = LLMEngine(EngineConfig(model="tiny-llama@2l", **kw),
                     ModelStage(cfg, 0, 2, "cpu", torch.float32).load_hf_state(sd))
    prompts = tf.prompts_of((3, 9, 20), cfg.vocab_size)
    got, exp = prefill_logits(eng, prompts), prefill_logits(want, prompts)
    # the same f32 weights through the same f32 ops: at most the last bits of a differently blocked matmul
    assert torch.allclose(got, exp, rtol=0, atol=1e-5 * exp.abs().max().item())


BASE = get_model_config("tiny-llama").to_hf_config()


@pytest.mark.parametrize("change,field", [
    ({"quant_method": "bitsandbytes"}, "quant_method"), ({"bits": 3}, "bits"), ({"bits": 8}, "bits"),
    ({"group_size": 64}, "group_size"), ({"group_size": -1}, "group_size"), ({"version": "gemv"}, "version"),
    ({"zero_point": False}, "zero_point"), ({"quant_method": "gptq", "desc_act": True}, "desc_act")])
def test_config_refuses_what_is_not_served(change, field):
    with pytest.raises(ValueError, match=field):
        ModelConfig.from_hf_config(dict(BASE, quantization_config=dict(QCONFIG["awq"], **change)))


@pytest.mark.parametrize("quant", ["none", "fp8"])
def test_other_quant_modes_refuse_the_checkpoint(tmp_path, quant):
    write_quantized(tmp_path / "m", "gptq")
    with pytest.raises(ValueError, match="int4"):
        LLMEngine(EngineConfig(model=str(tmp_path / "m"), quant=quant, device="cpu", dtype="float32"))
