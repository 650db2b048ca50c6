"""Multi-LoRA on the CPU: the reference contract, the row plan, adapter loading and its refusals,
the HostBatch section, and the engine path against merged weights (W + scale B A), which is
independent of the implementation."""
import json

import numpy as np
import pytest
import torch

import lora_cases as lc
from distributed_llms_amd import ops
from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.engine.batch import HostBatch, attach_lora, build_host_batch, merge_mixed, token_lora_slots
from distributed_llms_amd.engine.llm_engine import LLMEngine
from distributed_llms_amd.engine.sequence import SamplingParams
from distributed_llms_amd.models import lora as L
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.models.stage import ModelStage
from distributed_llms_amd.ops import reference as ref
from distributed_llms_amd.ops.lora import max_tiles, row_plan

NAME = "tiny-llama"
ADAPTERS = {"alpha": "synthetic:8:11", "beta": "synthetic:16:12:q_proj+v_proj+down_proj"}


# ------------------------------------------------------------------ contract on hand rows
def _hand():
    """3 rows, K = 2, packed slices of widths 2 and 1 (unequal), rp = 32 with rank 1."""
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0], [0.5, 4.0]])
    y0 = torch.tensor([[10.0, 20.0, 30.0], [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]])
    rp = 32
    a = torch.zeros(2, 2 * rp, 2)
    b = torch.zeros(2, 3, rp)
    # slot 0: slice 0 v = x0 + x1, B = [1, 2]; slice 1 v = x0 - x1, B = [3]
    a[0, 0] = torch.tensor([1.0, 1.0])
    a[0, rp] = torch.tensor([1.0, -1.0])
    b[0, 0, 0], b[0, 1, 0], b[0, 2, 0] = 1.0, 2.0, 3.0
    # slot 1: slice 0 only (slice 1 is a missing module: a zero slice); v = 2 x0, B = [1, -1]
    a[1, 0] = torch.tensor([2.0, 0.0])
    b[1, 0, 0], b[1, 1, 0] = 1.0, -1.0
    return x, y0, a, b


def test_contract_hand_rows():
    x, y0, a, b = _hand()
    scale = torch.tensor([2.0, 0.5])
    y = ref.lora_apply(y0, x, torch.tensor([0, -1, 1]), a, b, scale, (0, 2))
    # row 0, slot 0: v = (3, -1); d = (3, 6, -3); y = y0 + 2 d
    assert y[0].tolist() == [16.0, 32.0, 24.0]
    # row 1 has no adapter: untouched
    assert torch.equal(y[1], y0[1])
    # row 2, slot 1: v = 1; d = (1, -1, 0): the missing module's column keeps y0
    assert y[2].tolist() == [-0.5, -2.5, -3.0]
    assert torch.equal(y0, _hand()[1]), "lora_apply must not write its input"


def test_contract_rounds_v_once_in_the_engine_dtype():
    x = torch.tensor([[1.0, 2.0 ** -9]], dtype=torch.bfloat16)
    a = torch.zeros(1, 32, 2, dtype=torch.bfloat16)
    a[0, 0] = torch.tensor([1.0, 1.0])
    b = torch.zeros(1, 1, 32, dtype=torch.bfloat16)
    b[0, 0, 0] = 256.0
    y0 = torch.zeros(1, 1, dtype=torch.bfloat16)
    y = ref.lora_apply(y0, x, torch.tensor([0]), a, b, torch.tensor([1.0]), (0,))
    assert y.item() == 256.0            # v = bf16(1 + 2^-9) = 1: the tail is rounded away before B


def test_scales():
    assert ref.lora_scale(16, 8) == 2.0
    assert ref.lora_scale(16, 64, use_rslora=True) == 2.0
    assert ref.lora_scale(16, 64) == 0.25
    assert [ref.lora_rank_pad(r) for r in (1, 8, 32, 33, 64)] == [32, 32, 32, 64, 64]
    with pytest.raises(ValueError):
        ref.lora_rank_pad(65)


# ------------------------------------------------------------------ exact-case preconditions
@pytest.mark.parametrize("t,k,rank,widths", [(1, 256, 1, (256, 128, 128)), (17, 256, 8, (256, 128, 48)),
                                             (33, 4096, 64, (256, 128, 128)), (15, 4096, 16, (272,))])
def test_exact_case_preconditions_and_reference(t, k, rank, widths):
    c = lc.int_case(t, k, rank, widths)
    assert c.rounded >= lc.MIN_ROUNDED and c.ties >= lc.MIN_TIES
    assert c.v.abs().max().item() <= lc.V_LIMIT
    # the engine's reference on these inputs is the fp64 expectation, bit for bit
    y = ref.lora_apply(c.y0, c.x, c.slot, c.a, c.b, c.scale, c.starts)
    assert torch.equal(y, c.expected)
    assert torch.equal(y[c.slot < 0], c.y0[c.slot < 0])


def test_random_case_bound_holds_for_the_reference():
    c = lc.random_case(33, 256, 8, (256, 128, 48))
    y = ref.lora_apply(c.y0, c.x, c.slot, c.a, c.b, c.scale, c.starts)
    err = (y.to(torch.float64) - c.expected).abs()
    assert bool((err <= c.rounded).all())


# ------------------------------------------------------------------ row plan
def _brute_plan(slots):
    tiles = []
    for s in sorted(set(int(v) for v in slots if v >= 0)):
        rows = [i for i, v in enumerate(slots) if v == s]
        for i in range(0, len(rows), 16):
            tiles.append((s, rows[i:i + 16]))
    return tiles


@pytest.mark.parametrize("seed", range(6))
def test_row_plan_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    t, nslots = int(rng.integers(1, 200)), int(rng.integers(1, 9))
    slots = rng.integers(-1, nslots, size=t).astype(np.int32)
    tile_slot, tile_rows = row_plan(slots)
    nt = tile_slot.shape[0]
    assert nt <= max_tiles(t, nslots) and tile_rows.shape == (nt * 16,)
    want = _brute_plan(slots)
    assert nt == len(want)
    for i, (s, rows) in enumerate(want):
        assert tile_slot[i] == s
        got = tile_rows[i * 16:(i + 1) * 16]
        assert got[:len(rows)].tolist() == rows and (got[len(rows):] == -1).all()
    live = tile_rows[tile_rows >= 0]
    assert sorted(live.tolist()) == np.flatnonzero(slots >= 0).tolist()      # each adapter row exactly once
    # padded plan: unused tiles have slot -1 and no rows
    ps, pr = row_plan(slots, max_tiles(t, nslots))
    assert (ps[nt:] == -1).all() and (pr[nt * 16:] == -1).all() and (ps[:nt] == tile_slot).all()


def test_row_plan_no_adapter_rows():
    s, r = row_plan(np.full(5, -1, np.int32))
    assert s.shape == (0,) and r.shape == (0,)


# ------------------------------------------------------------------ PEFT directory
def _write_peft(path, cfg, rank=4, targets=("q_proj", "down_proj"), alpha=8, layers=None, **extra):
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(3)
    sd = {}
    for l in (range(cfg.num_layers) if layers is None else layers):
        for m in targets:
            n, k = L._module_shape(cfg, m)
            p = f"base_model.model.model.layers.{l}.{L._HF_PATH[m]}."
            sd[p + "lora_A.weight"] = torch.randn(rank, k, generator=g)
            sd[p + "lora_B.weight"] = torch.randn(n, rank, generator=g)
    path.mkdir(exist_ok=True)
    save_file(sd, str(path / "adapter_model.safetensors"))
    conf = {"peft_type": "LORA", "r": rank, "lora_alpha": alpha, "target_modules": list(targets), "bias": "none"}
    conf.update(extra)
    (path / "adapter_config.json").write_text(json.dumps(conf))
    return sd


def test_peft_directory_loads_tensor_equal(tmp_path):
    cfg = get_model_config(NAME)
    sd = _write_peft(tmp_path / "ad", cfg, use_rslora=True)
    ad = L.load_adapter("x", str(tmp_path / "ad"), cfg, 64)
    assert ad.rank == 4 and ad.scale == 8 / 2.0 and ad.targets == ("q_proj", "down_proj")
    for l in range(cfg.num_layers):
        for m in ("q_proj", "down_proj"):
            a, b = ad.factors(l, m)
            p = f"base_model.model.model.layers.{l}.{L._HF_PATH[m]}."
            assert torch.equal(a, sd[p + "lora_A.weight"]) and torch.equal(b, sd[p + "lora_B.weight"])
        assert ad.factors(l, "k_proj") is None
    # through a stage: slot tensors hold the factors zero-padded, the untargeted slices zero
    st = ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).init_synthetic(0)
    st.load_lora(EngineConfig(model=NAME, dtype="float32", device="cpu", lora_modules={"x": str(tmp_path / "ad")}))
    w = st.lora.layers[1]["wqkv"]
    assert w.starts == (0, cfg.q_size, cfg.q_size + cfg.kv_size) and w.a.shape == (1, 96, cfg.hidden_size)
    p = "base_model.model.model.layers.1.self_attn.q_proj."
    assert torch.equal(w.a[0, :4], sd[p + "lora_A.weight"]) and not w.a[0, 4:].any()
    assert torch.equal(w.b[0, :cfg.q_size, :4], sd[p + "lora_B.weight"]) and not w.b[0, cfg.q_size:].any()
    assert "wo" not in st.lora.layers[1] and "w_gate_up" not in st.lora.layers[1]


@pytest.mark.parametrize("kw,msg", [
    (dict(targets=("q_proj",), extra=dict(target_modules=["q_proj", "lm_head"])), "lm_head"),
    (dict(extra=dict(target_modules=["embed_tokens"])), "embed_tokens"),
    (dict(extra=dict(target_modules=["w1"])), "w1"),
    (dict(extra=dict(modules_to_save=["lm_head"])), "modules_to_save"),
    (dict(extra=dict(bias="all")), "bias"),
    (dict(extra=dict(use_dora=True)), "DoRA"),
    (dict(rank=16), "max_lora_rank"),
])
def test_peft_refusals(tmp_path, kw, msg):
    cfg = get_model_config(NAME)
    _write_peft(tmp_path / "ad", cfg, rank=kw.get("rank", 4), targets=kw.get("targets", ("q_proj", "down_proj")),
                **kw.get("extra", {}))
    with pytest.raises(ValueError, match=msg):
        L.load_adapter("x", str(tmp_path / "ad"), cfg, 8)


def test_engine_refusals(tmp_path, monkeypatch):
    lm = {"a": "synthetic:8:1"}
    with pytest.raises(ValueError, match="GPT-2"):
        LLMEngine(EngineConfig(model="tiny-gpt2", dtype="float32", device="cpu", lora_modules=lm))
    with pytest.raises(ValueError, match="quant"):
        LLMEngine(EngineConfig(model=NAME, dtype="float32", device="cpu", quant="fp8", lora_modules=lm))
    with pytest.raises(ValueError, match="tensor parallelism"):
        EngineConfig(model=NAME, lora_modules=lm).check_tensor_parallel(2)
    EngineConfig(model=NAME, lora_modules=lm).check_tensor_parallel(1)
    with pytest.raises(ValueError, match="Mixtral"):
        LLMEngine(EngineConfig(model="tiny-mixtral", dtype="float32", device="cpu",
                               lora_modules={"a": "synthetic:8:1:q_proj+gate_proj"}))
    with pytest.raises(ValueError, match="max_lora_rank"):
        LLMEngine(EngineConfig(model=NAME, dtype="float32", device="cpu", max_lora_rank=4, lora_modules=lm))
    monkeypatch.setenv("DLLM_PP_FINE", "1")
    with pytest.raises(ValueError, match="DLLM_PP_FINE"):
        LLMEngine(EngineConfig(model=NAME, dtype="float32", device="cpu", lora_modules=lm))


# ------------------------------------------------------------------ HostBatch
def _engine(lora=ADAPTERS, **kw):
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    args = dict(model=NAME, dtype="float32", device="cpu", max_batch=8, max_seq_len=256, use_graphs=False,
                num_kv_blocks=128, lora_modules=dict(lora or {}))
    args.update(kw)
    return LLMEngine(EngineConfig(**args), ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32).load_hf_state(sd))


PROMPTS = [[1, 5, 9, 200, 37, 44], [3, 4, 7], list(range(10, 50))]
WHO = [None, "alpha", "beta"]


def _params(adapter, n=8):
    return SamplingParams(max_new_tokens=n, ignore_eos=True, adapter=adapter)


def test_hostbatch_section_roundtrip_and_identity():
    eng = _engine()
    for p in PROMPTS:
        eng.add_request(p, _params(None))
    hb = build_host_batch(eng.scheduler.schedule(0), eng.bm, 32)
    assert hb.lora is None
    base = hb.pack().copy()
    assert base[13] == 0
    # the same batch with an adapter on one row: a section at the end, everything before it unchanged
    class S:
        def __init__(self, slot):
            self.lora_slot = slot
    attach_lora(hb, [S(-1), S(-1), S(-1)])
    assert hb.lora is None and np.array_equal(hb.pack(), base)      # no row asks: bytes identical
    attach_lora(hb, [S(-1), S(1), S(0)])
    packed = hb.pack()
    assert packed[13] == 1 and np.array_equal(packed[16:-3], base[16:]) and packed[-3:].tolist() == [-1, 1, 0]
    back = HostBatch.unpack(packed)
    assert back.lora.tolist() == [-1, 1, 0]
    assert token_lora_slots(back).tolist() == [-1] * 6 + [1] * 3 + [0] * 40


def test_hostbatch_native_decode_lookahead_and_mixed():
    eng = _engine(mixed_prefill_tokens=64)
    seqs = [eng.add_request(p, _params(w, n)) for p, w, n in zip(PROMPTS, WHO, (4, 2, 4))]
    eng.step()                                    # prefill
    st = eng.scheduler.schedule(0)                # natively packed decode step
    assert st.packed is not None and st.lora
    hb = build_host_batch(st, eng.bm, 32, eng.runner.max_blocks)
    assert hb.lora.tolist() == [s.lora_slot for s in st.seqs] and sorted(hb.lora.tolist()) == [-1, 0, 1]
    assert HostBatch.unpack(hb.pack()).lora.tolist() == hb.lora.tolist()
    # a lookahead step built while that one is in flight: the row that finishes by length is left
    # out (keep), the others keep their adapters
    la = eng.scheduler.schedule_lookahead(0)
    assert la is not None and la.keep is not None and len(la.keep) == 2
    hbl = build_host_batch(la, eng.bm, 32, eng.runner.max_blocks)
    assert hbl.lora.tolist() == [s.lora_slot for s in la.seqs] == [hb.lora[i] for i in la.keep]
    toks = eng.runner.execute(hb).argmax(-1).numpy()
    eng.scheduler.complete(st, toks)
    hbl.ids[:] = toks[la.keep]
    eng.scheduler.complete(la, eng.runner.execute(hbl).argmax(-1).numpy())
    # a mixed step: decode rows first, then the new prompt's chunk
    eng.add_request([7, 8, 9, 10], _params("beta", 2))
    mx = eng.scheduler.schedule(0)
    assert mx.mixed
    hbm = build_host_batch(mx, eng.bm, 32)
    nd = hbm.num_decode
    assert hbm.lora[:nd].tolist() == [s.lora_slot for s in mx.decode_seqs] and hbm.lora[nd:].tolist() == [1]
    assert token_lora_slots(hbm).tolist() == hbm.lora[:nd].tolist() + [1] * 4
    assert all(s.lora_slot == eng.adapter_slots[w] if w else s.lora_slot == -1 for s, w in zip(seqs, WHO))


def test_merge_mixed_one_side_without_adapter():
    z = np.zeros
    dec = HostBatch(False, z(2, np.int32), z(2, np.int32), z(2, np.int32), np.ones(2, np.int32),
                    np.arange(3, dtype=np.int32), z((2, 1), np.int32), np.arange(2, dtype=np.int32), 1, 1)
    pre = HostBatch(True, z(3, np.int32), z(3, np.int32), z(3, np.int32), np.array([3], np.int32),
                    np.array([0, 3], np.int32), z((1, 1), np.int32), np.array([2], np.int32), 3, 3,
                    lora=np.array([2], np.int32))
    assert merge_mixed(dec, pre, 0, 0).lora.tolist() == [-1, -1, 2]
    pre.lora = None
    assert merge_mixed(dec, pre, 0, 0).lora is None


# ------------------------------------------------------------------ semantics: merged weights
def _merged_state(cfg, sd, spec, dtype=torch.float32):
    """The HF state dict of W + scale B A for the synthetic adapter ``spec``."""
    ad = L.load_adapter("m", spec, cfg, 64)
    out = dict(sd)
    for l in range(cfg.num_layers):
        for m in ad.targets:
            a, b = ad.factors(l, m)
            key = f"model.layers.{l}.{L._HF_PATH[m]}.weight"
            out[key] = (sd[key].double() + ad.scale * (b.double() @ a.double())).to(dtype)
    return out


def _prefill_logits(eng, prompts, who):
    for p, w in zip(prompts, who):
        eng.add_request(p, SamplingParams(max_new_tokens=1, adapter=w))
    st = eng.scheduler.schedule(0)
    out = eng.runner.execute(build_host_batch(st, eng.bm, 32)).float()
    eng.scheduler.complete(st, out.argmax(-1).numpy())
    eng.run_until_done()
    return out


def test_adapter_engine_matches_merged_weights():
    """Fails without the feature: the adapter engine must compute what W + scale B A computes."""
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    eng = _engine({"alpha": ADAPTERS["alpha"]})
    merged = LLMEngine(EngineConfig(model=NAME, dtype="float32", device="cpu", max_batch=8, max_seq_len=256,
                                    use_graphs=False, num_kv_blocks=128),
                       ModelStage(cfg, 0, cfg.num_layers, "cpu", torch.float32)
                       .load_hf_state(_merged_state(cfg, sd, ADAPTERS["alpha"])))
    base = _engine(None)
    la = _prefill_logits(eng, PROMPTS, ["alpha"] * 3)
    lm = _prefill_logits(merged, PROMPTS, [None] * 3)
    lb = _prefill_logits(base, PROMPTS, [None] * 3)
    torch.testing.assert_close(la, lm, atol=1e-4, rtol=1e-4)
    assert (la - lb).abs().max().item() > 1e-2, "the adapter must change the logits"
    ta = eng.generate(PROMPTS, _params("alpha"))
    tm = merged.generate(PROMPTS, _params(None))
    assert ta == tm and all(len(t) == 8 for t in ta)
    assert ta != base.generate(PROMPTS, _params(None))


def test_adapter_engine_matches_transformers_on_merged_weights():
    transformers = pytest.importorskip("transformers")
    cfg = get_model_config(NAME)
    sd = W.synth_hf_state_dict(cfg, seed=5, dtype=torch.float32)
    hf_cfg = transformers.LlamaConfig(**{k: v for k, v in cfg.to_hf_config().items() if not k.startswith("_")
                                         and k not in ("model_type", "architectures")})
    model = transformers.LlamaForCausalLM(hf_cfg).eval()
    model.load_state_dict(_merged_state(cfg, sd, ADAPTERS["alpha"]), strict=True)
    eng = _engine({"alpha": ADAPTERS["alpha"]})
    prompt = PROMPTS[2]
    with torch.no_grad():
        want = model(torch.tensor([prompt])).logits[0, -1].float()
    got = _prefill_logits(eng, [prompt], ["alpha"])[0]
    torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------ engine: mixed requests
def _alone(kw, prompt, who, n=6):
    return _engine(**kw).generate([prompt], _params(who, n))[0]


@pytest.mark.parametrize("kw", [dict(), dict(max_prefill_tokens=16, mixed_prefill_tokens=0),
                                dict(mixed_prefill_tokens=16, max_prefill_tokens=64)],
                         ids=["whole", "chunked", "mixed"])
def test_mixed_requests_equal_each_alone(kw):
    eng = _engine(**kw)
    seqs = [eng.add_request(p, _params(w, 6)) for p, w in zip(PROMPTS[:2], WHO[:2])]
    eng.step()
    seqs.append(eng.add_request(PROMPTS[2], _params(WHO[2], 6)))     # arrives while the others decode
    eng.run_until_done()
    for s, p, w in zip(seqs, PROMPTS, WHO):
        assert s.output == _alone(kw, p, w), (w, kw)
    outs = [s.output for s in seqs]
    assert outs[1] != _alone(kw, PROMPTS[1], None), "the adapter must change the tokens"


def test_preempted_adapter_request_keeps_its_adapter():
    """A pool of three usable blocks: both prompts fill one, both need a second while decoding, the
    younger is preempted and recomputed -- with its adapter."""
    kw = dict(num_kv_blocks=4)
    prompts = [list(range(1, 31)), list(range(40, 71))]
    who = ["alpha", "beta"]
    eng = _engine(**kw)
    seqs = [eng.add_request(p, _params(w, 6)) for p, w in zip(prompts, who)]
    eng.run_until_done()
    assert eng.scheduler.num_preemptions > 0
    for s, p, w in zip(seqs, prompts, who):
        assert s.output == _alone(kw, p, w), w


def test_unknown_adapter_is_refused_at_add_request():
    eng = _engine()
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.add_request([1, 2], _params("gamma"))
    with pytest.raises(ValueError, match="unknown adapter"):
        _engine(None).add_request([1, 2], _params("alpha"))
    assert SamplingParams.from_dict(_params("alpha").to_dict()).adapter == "alpha"


def test_prefix_cache_ignores_adapter_requests():
    eng = _engine(enable_prefix_caching=True)
    prompt = list(range(1, 100))
    for _ in range(2):
        eng.generate([prompt], _params("alpha", 2))
    st = eng.scheduler.prefix_stats()
    assert st["query_tokens"] == 0 and st["hit_tokens"] == 0 and st["cached_blocks"] == 0
    # base requests still share
    for _ in range(2):
        eng.generate([prompt], _params(None, 2))
    st = eng.scheduler.prefix_stats()
    assert st["hit_tokens"] > 0 and st["cached_blocks"] > 0
    # and an adapter request takes nothing from what they registered
    before = eng.scheduler.prefix_stats()
    seq = eng.add_request(prompt, _params("beta", 2))
    eng.run_until_done()
    assert eng.scheduler.prefix_stats() == before and seq.cached_tokens == 0


def test_no_adapter_request_calls_no_lora_op(monkeypatch):
    calls = []
    real = ops.lora.apply
    monkeypatch.setattr(ops.lora, "apply", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops.lora, "make_plan", lambda *a, **k: calls.append(2))
    eng = _engine()
    want = _engine(None).generate(PROMPTS, _params(None))
    assert eng.generate(PROMPTS, _params(None)) == want and not calls
    monkeypatch.undo()
    monkeypatch.setattr(ops.lora, "apply", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    eng.generate(PROMPTS[:1], _params("alpha", 2))
    assert calls, "the counter must see the adapter path"
