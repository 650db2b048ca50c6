"""What models/stage.py asks of ``ops``, call by call, against a table recorded before the stage's host path was
consolidated (one projection helper, one pre-norm, one final norm).

tests/golden/stage_traces.json holds, for the grid below, every call the stage's forward made through ``ops`` (each
distinct call once, a case as the list of its calls' indices): the op,
which weight it got (layer and dict key, found by identity), the shapes and classes of its tensor arguments, and the
``bias`` / ``defer`` / ``quant_out`` it was given.  The harness wraps the attributes of ``ops`` that stage.py reaches
(and ``ops.lora.apply``); each wrapper records and calls through, so the ops run for real on CPU tensors.  Only calls
made from the stage are recorded, not what an op calls inside itself: the table pins the stage's host path, not the
ops'.  ``python tests/test_stage_trace.py --record`` rewrites the table from whatever tree it runs in.

Every case runs four steps: a prefill (``logits_idx``), a decode step, a mixed step, a prefill with ``score_idx``.
Tensor-parallel branches are left to tests/test_tensor_parallel.py, split-K partials (CUDA only) to the GPU suite."""
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

from distributed_llms_amd import knobs, ops
from distributed_llms_amd.config import EngineConfig, get_model_config
from distributed_llms_amd.engine.batch import build_host_batch, to_device_meta
from distributed_llms_amd.engine.llm_engine import make_block_manager
from distributed_llms_amd.engine.scheduler import Scheduler
from distributed_llms_amd.engine.sequence import SamplingParams, Sequence
from distributed_llms_amd.models.stage import ModelStage

TABLE = os.path.join(os.path.dirname(__file__), "golden", "stage_traces.json")
OPS = ["embedding", "rms_norm", "fused_add_rms_norm", "layer_norm", "linear", "linear_swiglu", "silu_mul", "gelu_tanh",
       "add_", "qkv_prep_", "moe_forward", "lm_head_logprobs", "rope_cache_append", "paged_attention_decode",
       "paged_attention_prefill", "paged_attention_decode_rope", "paged_attention_prefill_rope"]
FLAGS = ("bias", "defer", "quant_out")
LAYERS = 2                                  # every preset at two layers: the cuts below fall inside layer 1
ADAPTER = {"a": "synthetic:4:1"}            # all the projections the model can carry LoRA on

# (preset, quant, lora, pad_heads, cut): cut = the atom at which two stages split the model (unit_group 5), or None
CONFIGS = [("tiny-llama", q, False, False, None) for q in ("none", "fp8", "int4")] + \
          [("tiny-llama", "none", True, False, None), ("tiny-qwen2", "none", False, False, None),
           ("tiny-qwen2", "none", True, False, None), ("tiny-qwen3-d128", "none", False, False, None),
           ("tiny-qwen2-g7", "none", False, True, None), ("tiny-mixtral", "none", False, False, None),
           ("tiny-mixtral", "fp8", False, False, None), ("tiny-gpt2", "none", False, False, None)] + \
          [("tiny-llama", q, False, False, c) for q in ("none", "fp8") for c in range(5, 10)] + \
          [("tiny-gpt2", "none", False, False, 5)]       # GPT-2's hand-off between two stages, at the layer boundary
KNOBS = list(itertools.product((False, True), (False, True)))      # defer_qkv, defer_o


def config_id(c):
    preset, quant, lora, pad, cut = c
    return f"{preset}|{quant}" + ("|lora" if lora else "") + ("|pad" if pad else "") + (f"|cut{cut}" if cut else "")


def build_stages(c):
    preset, quant, lora, pad, cut = c
    spec = f"{preset}@{LAYERS}l"
    cfg = get_model_config(spec)
    n = 5 * cfg.num_layers
    stages = []
    for a, b in ([(0, n)] if cut is None else [(0, cut), (cut, n)]):
        st = ModelStage(cfg, 0, 0, "cpu", torch.float32, units=(a, b), unit_group=5,
                        pad_heads=True if pad else None).init_synthetic(3).quantize(quant)
        if lora:
            st.load_lora(EngineConfig(model=spec, device="cpu", dtype="float32", lora_modules=dict(ADAPTER)))
        stages.append(st)
    return stages


class Tracer:
    """Wraps the ops for one drive; ``out`` is the trace."""

    def __init__(self, stages):
        self.out, self.depth, self.names = [], 0, {}
        for si, st in enumerate(stages):
            pre = f"s{si}." if len(stages) > 1 else ""
            for i, lw in enumerate(st.layers):
                for k, t in lw.items():
                    self.names[id(t)] = f"{pre}L{st.layer_start + i}.{k}"
                if st.lora is not None:
                    for k, t in st.lora.layers[i].items():
                        self.names[id(t)] = f"{pre}L{st.layer_start + i}.lora.{k}"
            for k, t in list(st.embed.items()) + list(st.head.items()):
                self.names[id(t)] = pre + k
            if st.is_last:
                self.names[id(st.lm_head_weight())] = pre + "lm_head"
        self.saved = {}

    def entry(self, name, sig, a, kw):
        ba = sig.bind(*a, **kw)
        ba.apply_defaults()
        parts = []
        for p, v in ba.arguments.items():
            if id(v) in self.names:
                parts.append(f"{p}={self.names[id(v)]}")
            elif hasattr(v, "shape"):
                parts.append(f"{p}={type(v).__name__}{list(v.shape)}")
            elif p in FLAGS:
                parts.append(f"{p}={v}")
        return f"{name}({', '.join(parts)})"

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapper(*a, **kw):
            if self.depth == 0:
                self.out.append(self.entry(name, sig, a, kw))
            self.depth += 1
            try:
                return fn(*a, **kw)
            finally:
                self.depth -= 1
        return wrapper

    def __enter__(self):
        for name in OPS:
            self.saved[name] = getattr(ops, name)
            setattr(ops, name, self.wrap(name, self.saved[name]))
        self.saved["lora.apply"] = ops.lora.apply
        ops.lora.apply = self.wrap("lora.apply", ops.lora.apply)
        return self

    def __exit__(self, *exc):
        ops.lora.apply = self.saved.pop("lora.apply")
        for name, f in self.saved.items():
            setattr(ops, name, f)


def drive(stages, lora):
    """The four steps through the chain of stages -> the trace."""
    for st in stages:
        st.allocate_kv(16, 32)
    bm = make_block_manager(16, 32)
    sch = Scheduler(bm, 1, 4, 1024, 128, 64)

    def seq(prompt, new, score=False, slot=-1):
        return Sequence(prompt, SamplingParams(max_new_tokens=new, ignore_eos=True, prompt_logprobs=score),
                        lora_slot=slot)

    arrivals = [[seq([3, 4, 5, 6, 7], 3, slot=0 if lora else -1), seq([9, 9], 3)],     # prefill
                [],                                                                    # decode
                [seq([5, 6, 7], 1)],                                                   # mixed: finishes all three
                [seq([8, 7, 6, 5], 1, score=True, slot=0 if lora else -1)]]            # prefill that scores
    kinds = []
    with Tracer(stages) as tr:
        for new in arrivals:
            for s in new:
                sch.add(s)
            step = sch.schedule(0)
            ids, meta = to_device_meta(build_host_batch(step, bm, 32), "cpu")
            kinds.append((meta.is_prefill, meta.num_decode > 0, meta.logits_idx is not None, meta.score_idx is not None))
            tr.out.append(f"-- step: {meta.num_tokens} tokens")
            x = ids
            for st in stages:
                x = st.forward(x, meta)
            plp = None if meta.prompt_lp is None else meta.prompt_lp.numpy()
            sch.complete(step, x.argmax(-1).to(torch.int32).numpy(), 0.0, None, plp)
            sch.pop_finished()
    assert kinds == [(True, False, True, False), (False, False, False, False), (True, True, True, False),
                     (True, False, True, True)], kinds
    return tr.out


def run_config(c):
    """{"dq,do": trace} over the knob grid."""
    stages = build_stages(c)
    out = {}
    for dq, do in KNOBS:
        with knobs.override(defer_qkv=dq, defer_o=do):
            out[f"defer_qkv={int(dq)},defer_o={int(do)}"] = drive(stages, c[2])
    return out


@pytest.fixture(scope="module")
def shipped_knobs():
    saved = knobs.as_dict()
    knobs.update(knobs.Knobs().__dict__)     # a DLLM_KNOBS override in the environment cannot move the table
    yield
    knobs.update(saved)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_the_grid(table):
    assert sorted(table["cases"]) == sorted(f"{config_id(c)}|defer_qkv={int(q)},defer_o={int(o)}"
                                            for c in CONFIGS for q, o in KNOBS)
    used = {e.split("(")[0] for e in table["entries"]}
    assert used >= set(OPS) - {"paged_attention_decode_rope", "paged_attention_prefill_rope"} | {"lora.apply"}
    # the knobs move the dense Llama traces, and nothing where a bias, a q/k norm or adapter rows forbid a partial
    t = lambda cid, k: table["cases"][f"{cid}|{k}"]
    assert t("tiny-llama|none", "defer_qkv=0,defer_o=0") != t("tiny-llama|none", "defer_qkv=1,defer_o=0")
    assert t("tiny-llama|none", "defer_qkv=0,defer_o=0") != t("tiny-llama|none", "defer_qkv=0,defer_o=1")
    assert t("tiny-gpt2|none", "defer_qkv=0,defer_o=0") == t("tiny-gpt2|none", "defer_qkv=1,defer_o=1")


@pytest.mark.parametrize("c", CONFIGS, ids=config_id)
def test_stage_makes_the_recorded_calls(c, table, shipped_knobs):
    for k, trace in run_config(c).items():
        want = [table["entries"][i] for i in table["cases"][f"{config_id(c)}|{k}"]]
        assert trace == want, (config_id(c), k, next((a, b) for a, b in zip(trace + [None], want + [None]) if a != b))


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    knobs.update(knobs.Knobs().__dict__)
    entries, cases = {}, {}                  # every distinct call is stored once; a case is a list of indices
    for c in CONFIGS:
        for k, trace in run_config(c).items():
            cases[f"{config_id(c)}|{k}"] = [entries.setdefault(e, len(entries)) for e in trace]
    with open(TABLE, "w") as f:
        f.write('{"entries": [\n' + ",\n".join(json.dumps(e) for e in entries) + '\n],\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()))
        f.write("\n}}\n")
    print(len(cases), "cases,", len(entries), "entries,", os.path.getsize(TABLE), "bytes")
