"""Imported 4-bit checkpoints on the GPU: ``w4_repack`` (csrc/kernels/w4_repack.hip) against the CPU path bit for bit,
the zero-point variants of ``gemm_w4a16`` / ``dequant_w4`` (csrc/kernels/gemm_w4.hip) against exact fp64, and a
quantized checkpoint directory through the bf16 engine against the float32 CPU engine."""
import gc

import pytest
import torch

import teacher_forced as tf
import test_int4_gpu as base
from test_int4_import import FORMATS, checkpoint, random_weight, write_quantized
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.ops import gemm, int4, reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("n,k", [(128, 128), (256, 384)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_w4_repack_matches_the_cpu_path_and_stays_in_its_rows(fmt, n, k):
    parts = checkpoint(fmt, *random_weight(n, k, seed=n + k))
    want = int4.from_checkpoint([parts], fmt)
    parts = tuple(t.to(DEV) for t in parts)
    fill = lambda width: torch.full((24, k // 128, width), 0xA5, dtype=torch.uint8, device=DEV)
    dst = int4.Int4Weight(fill(1024), fill(64).view(torch.int32))           # 384 rows
    int4.repack_into(dst, 128, *parts, fmt)
    for got, exp in ((dst.packed.cpu(), want.packed), (dst.sz.cpu().view(torch.uint8), want.sz.view(torch.uint8))):
        assert torch.equal(got[8:8 + n // 16], exp)
        assert (got[:8] == 0xA5).all() and (got[8 + n // 16:] == 0xA5).all()
    w = int4.from_checkpoint([parts, parts], fmt)
    assert torch.equal(w.packed.cpu(), want.packed.repeat(2, 1, 1)) and torch.equal(w.sz.cpu(), want.sz.repeat(2, 1, 1))
    assert torch.equal(w.scales().cpu(), want.scales().repeat(2, 1)) and torch.equal(w.zeros().cpu(), want.zeros().repeat(2, 1))


@pytest.mark.parametrize("n,k", [(128, 256), (256, 512)])
@pytest.mark.parametrize("m", [1, 17, 64, 65])
def test_zero_point_gemm_is_exact_and_repeatable(m, n, k):
    """Integer x in [-4, 4], power-of-two scales 2^-4 .. 2^2, code - zero in [-15, 15]: every partial sum is a
    multiple of 2^-4 below 2^18, exact in f32 in any order, so the only rounding is the one to bf16."""
    u, z, s = random_weight(n, k, seed=m + n, pow2=True)
    w = int4.from_codes(u, s, z).to(DEV)
    x = torch.randint(-4, 5, (m, k), generator=torch.Generator().manual_seed(m)).double()
    want = (x @ ref.dequantize_w4(u, s, z).double().t()).to(torch.bfloat16)
    xg = x.to(DEV, torch.bfloat16)
    for splits in (1, 2, 0):
        y = base._run(xg, w, splits)
        assert torch.equal(y, want), splits
        assert torch.equal(base._run(xg, w, splits), y)


def test_zero_point_dequant_is_the_host_inverse_and_its_route_the_bf16_gemm():
    u, z, s = random_weight(256, 384, seed=3)
    host = int4.from_codes(u, s, z)
    w = host.to(DEV)
    wd = int4.dequant(w)
    assert torch.equal(wd.cpu(), host.dequantize(torch.bfloat16))
    x = torch.randn(5, 384, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16)
    assert torch.equal(int4.linear_int4(x, w, dequant_min_m=1), gemm.linear(x, wd))


@pytest.mark.parametrize("m,n,k,dequant", [(5, 128, 256, False), (200, 384, 1024, False), (300, 384, 1024, True)])
def test_random_data_meets_the_symmetric_kernel_rule(monkeypatch, m, n, k, dequant):
    """The random case of tests/test_int4_gpu.py itself, handed an asymmetric f16-scale weight."""
    def weight(n, k, seed, pow2=False):
        u, z, s = random_weight(n, k, seed, pow2)
        return int4.from_codes(u, s, z).to(DEV), ref.dequantize_w4(u, s, z).double()
    monkeypatch.setattr(base, "_weight", weight)
    base.test_random_within_the_f32_accumulation_bound(m, n, k, dequant)


def test_engine_serves_a_quantized_checkpoint_directory(tmp_path):
    """Greedy tokens against the float32 CPU engine, row by row on the tokens the GPU engine saw, where the CPU
    top-2 margin exceeds twice the per-row logit error tf.GPU_BOUNDS holds this model's bf16 engine to (no smaller
    error changes the arg-max).  The top-2 gap of 512 near-normal logits is about exponential with mean 0.28 spread:
    exp(-0.128 / 0.28) = 63 % of the rows should count, and at most half may be skipped.  Seed 7: the CPU engine
    alone, on its own greedy run, decides 19 of its 24 rows (seed 5: 17, seed 6: 15)."""
    write_quantized(tmp_path / "m", "awq", seed=7)
    kw = dict(model=str(tmp_path / "m"), quant="int4", max_batch=4, max_seq_len=64, num_kv_blocks=16)
    cpu = LLMEngine(EngineConfig(device="cpu", dtype="float32", **kw))
    eng = LLMEngine(EngineConfig(device=DEV, graph_batch_sizes=(1, 2, 4), **kw))
    assert all(lw["wqkv"].device.type == "cuda" and lw["wqkv"].zeros() is not None for lw in eng.stage.layers)
    rec = tf.record(eng)
    eng.generate(tf.prompts_of((5, 3, 7), 512), tf.greedy(8))
    recs = rec.finish()
    del eng, rec              # the engine and its graphs are gone before any other test captures one
    gc.collect()
    assert len(recs) == 3 * 8
    seen = [(list(r.seq.prompt) + list(r.seq.output))[:r.pos + 1] for r in recs]
    ref_rec = tf.record(cpu)
    cpu.generate(seen, tf.greedy(1))
    by_prompt = {tuple(r.seq.prompt): r.logits for r in ref_rec.finish()}
    want, got = torch.stack([by_prompt[tuple(s)] for s in seen]), torch.stack([r.logits for r in recs])
    top2 = want.topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * tf.GPU_BOUNDS["tiny-llama"].max * want.std()
    print(f"int4 import engine: {int(decided.sum())} of {len(recs)} rows decided, "
          f"max |logit error| / spread {((got - want).abs().max() / want.std()).item():.4f}")
    assert decided.float().mean() >= 0.5
    assert torch.equal(got.argmax(-1)[decided], want.argmax(-1)[decided])
