"""Int4 (W4A16) kernels on the GPU (csrc/kernels/gemm_w4.hip) against exact and fp64 references of the same codes
and scales (contract: ops/reference.py "int4 weights"), and the quant="int4" engine against the float32 CPU engine
on the dequantized weights.
"""
import gc

import pytest
import torch

import teacher_forced as tf
from distributed_llms_amd.config import EngineConfig
from distributed_llms_amd.engine.llm_engine import LLMEngine, build_stage
from distributed_llms_amd.ops import gemm, int4

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _weight(n, k, seed, pow2=False):
    """Random codes covering all 16 values and random bf16 scales (``pow2``: powers of two), on the GPU."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    u[:, :16] = torch.arange(16, dtype=torch.uint8)
    e = torch.randint(-4, 3, (n, k // 128), generator=g).float()
    s = torch.exp2(e) if pow2 else torch.exp2(e) * (1 + torch.rand(n, k // 128, generator=g))
    w = int4.from_codes(u, s.to(torch.bfloat16))
    return int4.Int4Weight(w.packed.to(DEV), w.scale.to(DEV)), w.dequantize(torch.float64)


def _run(x, w, splits, min_m=None):
    """The op with ``y`` between NaN guard rows and a NaN-filled workspace; the guards must survive."""
    m, n = x.shape[0], w.shape[0]
    gemm._workspace(x.device).fill_(NAN)
    buf = torch.full((m + 2, n), NAN, dtype=torch.bfloat16, device=DEV)
    if min_m is None:
        int4.linear_int4(x, w, splits_=splits, out=buf[1:m + 1])
    else:
        buf[1:m + 1] = int4.linear_int4(x, w, dequant_min_m=min_m)
    assert buf[0].isnan().all() and buf[m + 1].isnan().all()
    return buf[1:m + 1].cpu()


@pytest.mark.parametrize("k,n,splits", [(128, 128, 1), (128, 384, 1), (256, 128, 1), (256, 384, 2)])
def test_identity_returns_every_nibble(k, n, splits):
    w, wd = _weight(n, k, seed=k + n)
    y = _run(torch.eye(k, dtype=torch.bfloat16, device=DEV), w, splits)
    assert torch.equal(y, wd.float().to(torch.bfloat16).t())


@pytest.mark.parametrize("k", [128, 1024])
@pytest.mark.parametrize("m", [1, 63, 65, 256])
def test_selector_rows_are_exact_and_repeatable(m, k):
    n = 256
    w, wd = _weight(n, k, seed=m + k, pow2=True)
    g = torch.Generator().manual_seed(m)
    x = torch.zeros(m, k, dtype=torch.float64)
    rows = torch.arange(m)
    vals = torch.tensor([1., -1., 2., -2.], dtype=torch.float64)
    for _ in range(2):      # one or two non-zeros of +-1 / +-2 per row
        x[rows, torch.randint(0, k, (m,), generator=g)] = vals[torch.randint(0, 4, (m,), generator=g)]
    want = (x @ wd.t()).to(torch.bfloat16)
    xg = x.to(DEV, torch.bfloat16)
    for splits in (1, 4):
        y = _run(xg, w, splits)
        assert torch.equal(y, want), splits
        assert torch.equal(_run(xg, w, splits), y)


@pytest.mark.parametrize("m,n,k,dequant", [(5, 128, 256, False), (200, 384, 1024, False), (300, 384, 1024, False),
                                             (300, 384, 1024, True)])
def test_random_within_the_f32_accumulation_bound(m, n, k, dequant):
    w, wd = _weight(n, k, seed=m)
    g = torch.Generator().manual_seed(n + k)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    want = x.double() @ wd.t()
    mag = x.double().abs() @ wd.abs().t()
    # half a bf16 ulp of the exact result + K 2^-23 sum |x wd|; the dequant route rounds wd to bf16 once: + 2^-8 sum
    bound = torch.exp2(torch.frexp(want)[1].double() - 9) * (want != 0) + k * 2.0 ** -23 * mag
    if dequant:
        bound += 2.0 ** -8 * mag
    y = _run(x.to(DEV), w, 0, min_m=1 if dequant else 1 << 30).double()
    excess = ((y - want).abs() - bound).max().item()
    print(f"int4 random {m}x{n}x{k} dequant={dequant}: max |err| {(y - want).abs().max().item():.3e}, max (|err| - bound) {excess:.3e}")
    assert excess <= 0


@pytest.mark.parametrize("n,k", [(128, 128), (384, 1024)])
def test_dequant_w4_matches_the_host_inverse(n, k):
    w, _ = _weight(n, k, seed=7)
    assert torch.equal(int4.dequant(w).cpu(), int4.Int4Weight(w.packed.cpu(), w.scale.cpu()).dequantize(torch.bfloat16))


MODEL = "tiny-llama-d128"
_KW = dict(model=MODEL, max_batch=8, max_seq_len=128, num_kv_blocks=64, graph_batch_sizes=(1, 2, 4))
_shared = {}


def _mean_error(ecfg, stage, cpu):
    """Mean |logit error| of every prefill and decode row a GPU engine over ``stage`` runs on three prompts,
    teacher-forced: the reference of a row is the CPU engine's prefill logits of the tokens that row had seen.  The
    engine and its graphs are gone when this returns."""
    eng = LLMEngine(ecfg, stage)
    rec = tf.record(eng)
    eng.generate(tf.prompts_of((5, 3, 7), 1024), tf.greedy(5))
    recs = rec.finish()
    del eng, rec
    gc.collect()
    assert {r.kind for r in recs} > {"prefill"} and len(recs) == 3 * 5
    seen = [(list(r.seq.prompt) + list(r.seq.output))[:r.pos + 1] for r in recs]
    ref = tf.record(cpu)
    cpu.generate(seen, tf.greedy(1))
    want = {tuple(r.seq.prompt): r.logits for r in ref.finish()}
    return torch.stack([(r.logits - want[tuple(s)]).abs().mean() for r, s in zip(recs, seen)]).mean().item()


def _setup():
    """The int4 stage; its weights, dequantized, in a float32 CPU engine (the reference); and the error of a plain
    bf16 GPU engine on the same dequantized weights against it (the floor)."""
    if not _shared:
        q = build_stage(EngineConfig(**_KW, quant="int4"), device=DEV)
        assert sum(isinstance(t, int4.Int4Weight) for lw in q.layers for t in lw.values()) == 4 * len(q.layers) > 0
        made = {}
        for dev, dt in (("cpu", torch.float32), (DEV, torch.bfloat16)):
            ecfg = EngineConfig(**_KW, dtype=str(dt).split(".")[1], device=dev, use_graphs=dev != "cpu")
            st = build_stage(ecfg, device=dev)
            conv = lambda t: (t.dequantize(dt) if isinstance(t, int4.Int4Weight) else t.to(dt)).to(dev)
            st.layers = [{k: conv(t) for k, t in lw.items()} for lw in q.layers]
            st.embed, st.head = ({k: conv(t) for k, t in d.items()} for d in (q.embed, q.head))
            made[dev] = (ecfg, st)
        cpu = LLMEngine(*made["cpu"])
        _shared.update(q=q, cpu=cpu, floor=_mean_error(*made[DEV], cpu))
    return _shared


@pytest.mark.parametrize("graphs", [True, False])
def test_engine_logits_track_the_float32_engine_on_dequantized_weights(graphs):
    """Measured on an MI355X (profiles/int4.md): int4 engine 0.00269, plain bf16 engine 0.00294, graphs on and off."""
    e = _setup()
    err = _mean_error(EngineConfig(**_KW, quant="int4", use_graphs=graphs), e["q"], e["cpu"])
    print(f"int4 engine (graphs {graphs}): mean |logit error| {err:.5f}, plain bf16 engine {e['floor']:.5f}")
    assert err <= 1.35 * e["floor"]
